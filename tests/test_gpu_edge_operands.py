"""The operand contract of the per-op entries at their ragged edges: every row of tests/edge_rows.py runs with every operand -- inputs,
outputs, in/out tensors, scratch -- between bands inside one allocation (tests/guarded.py: 16 KiB for tensors, 1 MiB for a scratch cut
to exactly the queried size), under two band fills: N (0xFF, every word a NaN) and F (0x4B, every word large and finite: what a stray
read that flows through fmaxf, a clamp or a select becomes, which a NaN would not survive).  Outputs are NaN-filled before the call.

Per row and fill: rc 0 (a row is never skipped and never refused), every band intact, every input's payload bit-unchanged, every
floating output finite, and the float64 comparison the op's own test makes, at that test's tolerance; and the outputs bit-equal between
the two fills.  The loop is tests/guarded.py::run_row, shared with tests/test_gpu_scratch_contract.py.

The bands lie inside the test's own allocation: an access up to 16 KiB outside an operand lands in memory the test owns."""
import pytest

pytestmark = pytest.mark.gpu

import gpu_util as G                                             # noqa: E402
import guarded as GD                                             # noqa: E402
from edge_rows import ROWS                                       # noqa: E402
from sr3_hip import lib as L                                     # noqa: E402

FILLS = (('N', GD.N), ('F', GD.F))


@pytest.mark.parametrize('row', ROWS, ids=[r.id for r in ROWS])
def test_per_op_operand_contract(row):
    lib = L.load()
    refusal = row.spec().get('refusal')
    assert refusal is None or refusal(lib) is None, 'the row\'s own rule says it is refused: %s' % refusal(lib)
    GD.run_row(row, lib, G.dev(), G.stream(), fills=FILLS, operands=True)
