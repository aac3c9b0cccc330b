"""The refusals behind the scratch / workspace contract, CPU only: every entry that consumes a `*_scratch_bytes`, `*workspace_bytes` or
`*derived_bytes` query refuses a buffer one byte smaller than the query (naming both sizes) and a misaligned one, on the host, before
anything is launched -- no device is present here and every pointer is a made-up address that no case may touch.  An undersized buffer
is never handed to a kernel on a GPU: this is where that half of the contract is checked.  The completeness test keeps the two
tables (the per-op rows of tests/scratch_rows.py, the whole-plan entries below) in step with the symbol table of sr3_hip/lib.py."""
import ctypes as C
import re

import pytest

from scratch_rows import NOMEM, ALIGN, ROWS


def _p(k, off=0):
    """a made-up, 256-byte aligned, non-NULL address"""
    return C.c_void_p((k << 24) + off)


def _fake(spec):
    names = list(spec['ins']) + list(spec['outs'])
    P = {n: _p(i + 1) for i, n in enumerate(names)}
    if spec.get('derived'):
        P['derived'] = _p(len(names) + 1)
    return P, _p(len(names) + 2)


def _misalign(align):
    return align // 2


@pytest.mark.parametrize('row', ROWS, ids=[r.id for r in ROWS])
def test_per_op_scratch_is_checked_on_the_host(row):
    from sr3_hip import lib as L
    lib = L.load()
    spec = row.spec()
    nb = spec['query'](lib)
    assert nb > 0, 'the row has nothing in scratch'
    if spec.get('expect') is not None:
        assert nb == spec['expect'], (nb, spec['expect'])
    P, scratch = _fake(spec)
    if row.small is not None:
        least = spec.get('min_bytes', nb)
        assert spec['call'](lib, P, scratch, least - 1, None) == row.small, lib.sr3_last_error()
        msg = lib.sr3_last_error().decode()
        assert str(least - 1) in msg and re.search(r'\b%d\b' % least, msg), 'the refusal does not name both sizes: %r' % msg
    if row.align:
        bad = C.c_void_p(scratch.value + _misalign(row.align))
        assert spec['call'](lib, P, bad, nb, None) == ALIGN, (row.align, lib.sr3_last_error())
        assert 'align' in lib.sr3_last_error().decode()


# ---- the whole-plan entries ---------------------------------------------------------------------------------------------------------

def _plan():
    from sr3_hip import engine as E
    return E.Plan('sr3', 6, 3, 64, 32, [1, 2, 2], [8], 1, 32)


def _forward(plan, ws, nbytes, B=3):
    return plan.lib.sr3_unet_forward(plan.handle, _p(1), _p(2), 3, _p(3), None, _p(4), None, None, _p(5), ws, nbytes, _p(6), B, None)


def _reverse_step(plan, ws, nbytes, B=3):
    return plan.lib.sr3_reverse_step_hist(plan.handle, _p(1), _p(2), 3, _p(4), _p(3), _p(7), _p(5), ws, nbytes, _p(8), _p(9), _p(10), _p(11), _p(12),
                                          _p(13), 1, None, B, None, None, None, None)


def _train_step(plan, ws, nbytes, B=3):
    return plan.lib.sr3_train_step_ex(plan.handle, _p(1), _p(2), 3, _p(3), _p(4), _p(5), _p(6), None, _p(7), _p(8), _p(9), ws, nbytes, _p(10),
                                      1.0, 0.0, 0, 0, None, None, B, None, None, None, -1, 0.0, None)


PLAN_ENTRIES = {
    # entry: (its query, the launch)
    'sr3_unet_forward': ('sr3_workspace_bytes', _forward),
    'sr3_reverse_step_hist': ('sr3_workspace_bytes', _reverse_step),
    'sr3_train_step_ex': ('sr3_train_workspace_bytes', _train_step),
    'sr3_plan_bind_derived': ('sr3_plan_derived_bytes', lambda plan, buf, nbytes, B=3: plan.lib.sr3_plan_bind_derived(plan.handle, buf, nbytes)),
}


@pytest.mark.parametrize('entry', list(PLAN_ENTRIES))
@pytest.mark.parametrize('geometry', [(32, 32), (24, 40)], ids=['native', '24x40'])
def test_whole_plan_buffers_are_checked_on_the_host(entry, geometry):
    plan = _plan()
    plan.set_option('train_geom', 1)
    plan.set_geometry(*geometry)
    query, launch = PLAN_ENTRIES[entry]
    lib = plan.lib
    nb = {'sr3_workspace_bytes': lambda: plan.workspace_bytes(3), 'sr3_train_workspace_bytes': lambda: int(lib.sr3_train_workspace_bytes(plan.handle, 3, 3)),
          'sr3_plan_derived_bytes': lambda: int(lib.sr3_plan_derived_bytes(plan.handle))}[query]()
    assert nb > 0
    ws = _p(40)
    assert launch(plan, ws, nb - 1) == NOMEM, lib.sr3_last_error()
    msg = lib.sr3_last_error().decode()
    assert str(nb - 1) in msg and re.search(r'\b%d\b' % nb, msg), msg
    assert launch(plan, C.c_void_p(ws.value + (8 if entry == 'sr3_plan_bind_derived' else 128)), nb) == ALIGN, lib.sr3_last_error()
    assert 'align' in lib.sr3_last_error().decode()


def test_every_size_query_has_a_contract_row():
    """Every `*_scratch_bytes`, `*workspace_bytes` and `*derived_bytes` symbol of the binding appears in a table: a query someone adds
    cannot ship without a contract row; and every entry the header names as a consumer of sr3_conv_scratch_bytes has a row."""
    from sr3_hip import lib as L
    queries = set(n for n in L.SIGNATURES if re.search(r'(_scratch_bytes|workspace_bytes|derived_bytes)$', n))
    assert len(queries) >= 19
    tabled = set(r.query for r in ROWS) | set(q for q, _ in PLAN_ENTRIES.values())
    assert queries - tabled == set(), 'size queries without a contract row: %s' % sorted(queries - tabled)
    assert tabled - queries == set(), 'rows for queries the binding does not have: %s' % sorted(tabled - queries)
    for r in ROWS:
        assert r.entry in L.SIGNATURES, r.entry
    assert {'sr3_conv_f32', 'sr3_block_conv_f32', 'sr3_conv_dropout_f32'} <= set(r.entry for r in ROWS if r.query == 'sr3_conv_scratch_bytes')
    assert {'sr3_grad_norm', 'sr3_grad_accumulate'} <= set(r.entry for r in ROWS if r.query == 'sr3_grad_norm_scratch_bytes')
