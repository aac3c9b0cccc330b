"""The refusals of the training-step entries and of the two loss ops, byte for byte (CPU only: every case refuses before the first launch).

tests/golden/train_step_refusals.json holds, for every case of the tables below, the return code and the whole sr3_last_error() text,
recorded from the library as it was while each of sr3_train_step_ex / _ex2 / _ex3 forwarded its ~30 positional arguments to one body
with defaulted trailing parameters, before the entries filled one request struct.  Whatever checks that struct has to give the same code
and the same text for the same call, so also the same ORDER of checks: the two-fault cases say which of two faults is reported.

Record again (only from a library whose refusals are the wanted ones):  SR3_LIBRARY=/path/lib.so python tests/test_train_refusals_cpu.py
"""
import ctypes as C
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_step_refusals.json')
NAN, INF = float('nan'), float('inf')
B = 2


def _p(k, off=0):
    """a made-up, 256-byte aligned, non-NULL address: every case refuses before it touches memory"""
    return C.c_void_p((k << 24) + off)


WS = 64                      # the workspace's address number: the highest one, so that nothing lies behind it whatever its size
PLANS = {'sr3': ('sr3', 6, 3, 0), 'var': ('sr3', 6, 6, 3), 'ddpm': ('ddpm', 3, 3, 0)}      # variant, in_channel, out_channel, var_channels
_plans = {}


def _plan(name):
    """-> (plan, its training workspace bytes at batch B, the bytes of the per-image scratch at batch B)"""
    if name not in _plans:
        from sr3_hip import engine as E
        variant, cin, cout, var = PLANS[name]
        plan = E.Plan(variant, cin, cout, 8, 4, [1, 2], [8], 1, 16)
        if var:
            plan.set_option('var_channels', var)
        need = int(plan.lib.sr3_train_workspace_bytes(plan.handle, B, cin - 3))
        assert need > 0
        _plans[name] = (plan, need, int(plan.lib.sr3_vlb_terms_partials_bytes(B)))
    return _plans[name]


STEP_KEYS = ('hr', 'cond', 'cc', 'z', 'ca', 'cb', 'level', 'tstep', 'freq', 'params', 'grads', 'ws', 'ws_bytes', 'loss', 'grad_scale', 'dropout_p',
             'seed', 'n_marks', 'mark_offsets', 'mark_events', 'batch', 'tgt_z', 'tgt_x0', 'weight', 'kind', 'delta')
TAILS = {'sr3_train_step_ex': (), 'sr3_train_step_ex2': ('scal', 'lam', 'vlb'),
         'sr3_train_step_ex3': ('scal', 'lam', 'vlb', 'pi_out', 'pi_scratch', 'pi_bytes', 'vw')}
FLOATS = ('grad_scale', 'dropout_p', 'delta', 'lam', 'scale')


def _step_args(entry, plan='sr3', ws_short=0, pi_short=0, no_plan=False, **kw):
    """the arguments of one of the three entries on the plan `plan`: a call that would run, then `kw`.  ws_short / pi_short: that many
    bytes less than the workspace / the per-image scratch needs"""
    P, need, nb = _plan(plan)
    ddpm = plan == 'ddpm'
    a = dict(hr=_p(1), cond=None if ddpm else _p(2), cc=0 if ddpm else 3, z=_p(3), ca=_p(4), cb=_p(5), level=None if ddpm else _p(6),
             tstep=_p(7) if ddpm else None, freq=_p(8), params=_p(9), grads=_p(10), ws=_p(WS), ws_bytes=need - ws_short, loss=_p(11), grad_scale=1.0,
             dropout_p=0.0, seed=0, n_marks=0, mark_offsets=None, mark_events=None, batch=B, tgt_z=None, tgt_x0=None, weight=None, kind=-1, delta=0.0,
             scal=_p(12), lam=0.001, vlb=_p(13), pi_out=_p(14), pi_scratch=_p(15), pi_bytes=nb - pi_short, vw=None)
    a.update(kw)
    vals = [C.c_float(a[k]) if k in FLOATS else a[k] for k in STEP_KEYS + TAILS[entry]]
    return [None if no_plan else P.handle] + vals + [None]


def _tables(**kw):
    return dict(dict(tgt_z=_p(16), tgt_x0=_p(17), weight=_p(18)), **kw)


# what every one of the three entries refuses ...
COMMON = [dict(no_plan=True)] + [{k: None} for k in ('hr', 'z', 'ca', 'cb', 'freq', 'params', 'grads', 'ws', 'loss')] + [
    dict(tgt_z=_p(16)), dict(tgt_x0=_p(17)), dict(weight=_p(18)), dict(tgt_z=_p(16), tgt_x0=_p(17)), dict(tgt_z=_p(16), weight=_p(18)),
    dict(tgt_x0=_p(17), weight=_p(18)),
    dict(kind=-2), dict(kind=3), _tables(kind=3), dict(kind=2, delta=0.0), dict(kind=2, delta=NAN), _tables(kind=2, delta=0.0),
    dict(ws_short=1), dict(ws=_p(WS, 128)), dict(params=_p(9, 8)), dict(grads=_p(10, 4)),
    dict(level=None), dict(plan='ddpm', tstep=None), dict(dropout_p=1.0), dict(dropout_p=-0.5), dict(batch=0), dict(cc=6),
]
# ... on the plan that suits the entry (sr3_train_step_ex3 takes either)
ON = {'sr3_train_step_ex': ('sr3',), 'sr3_train_step_ex2': ('var',), 'sr3_train_step_ex3': ('sr3', 'var')}
EX_ONLY = [dict(plan='var')]                                                      # variance rows without step_scalars
EX2_ONLY = [dict(plan='var', scal=None), dict(plan='sr3'), dict(plan='var', lam=-1.0), dict(plan='var', lam=INF), dict(plan='var', lam=NAN)]
EX3_ONLY = [dict(scal=None), dict(plan='var', scal=None), dict(plan='var', lam=-1.0), dict(plan='var', lam=INF),
            dict(pi_scratch=None), dict(pi_short=1), dict(pi_out=_p(15)), dict(pi_out=_p(15, 8)), dict(pi_out=_p(WS)), dict(pi_scratch=_p(WS, 256)),
            dict(pi_scratch=_p(15, 4)), dict(plan='var', pi_scratch=None), dict(plan='var', pi_scratch=_p(15, 4))]

LOSS_KEYS = ('z', 'out', 'hr', 'tgt_z', 'tgt_x0', 'weight', 'batch', 'channels', 'pixels', 'kind', 'delta', 'scale', 'g', 'loss', 'scratch')
HYB_KEYS = ('z', 'out', 'hr', 'xt', 'tgt_z', 'tgt_x0', 'weight', 'scal', 'lam', 'batch', 'channels', 'pixels', 'kind', 'delta', 'scale', 'g', 'loss',
            'vlb', 'scratch')


def _loss_args(entry, **kw):
    a = dict(z=_p(1), out=_p(2), hr=_p(3), xt=_p(4), tgt_z=None, tgt_x0=None, weight=None, scal=_p(5), lam=0.001, batch=B, channels=3, pixels=16,
             kind=0, delta=1.0, scale=1.0, g=_p(6), loss=_p(7), vlb=_p(8), scratch=_p(9))
    a.update(kw)
    keys = LOSS_KEYS if entry == 'sr3_loss_grad_f32' else HYB_KEYS
    return [C.c_float(a[k]) if k in FLOATS else a[k] for k in keys] + [None]


LOSS_COMMON = [{k: None} for k in ('z', 'out', 'g', 'loss', 'scratch')] + [
    dict(tgt_z=_p(16)), dict(weight=_p(18)), dict(tgt_z=_p(16), tgt_x0=_p(17)), dict(tgt_x0=_p(17), weight=_p(18)),
    dict(kind=-1), dict(kind=3), dict(kind=2, delta=0.0), dict(kind=2, delta=NAN), _tables(kind=2, delta=INF),
    dict(batch=0), dict(pixels=0), dict(channels=0), dict(channels=5), dict(scratch=_p(9, 4)),
]
LOSS_ONLY = [_tables(hr=None)]
HYB_ONLY = [dict(hr=None), dict(xt=None), dict(scal=None), dict(lam=-1.0), dict(lam=INF), dict(lam=NAN)]

# two faults in one call: the one reported is the one the checks meet first
TWO_STEP = [
    ('sr3_train_step_ex2', dict(plan='var', scal=None, hr=None)), ('sr3_train_step_ex3', dict(scal=None, hr=None)),
    ('sr3_train_step_ex3', dict(scal=None, no_plan=True)),
    ('sr3_train_step_ex', dict(hr=None, kind=3)), ('sr3_train_step_ex', dict(kind=3, ws_short=1)), ('sr3_train_step_ex', dict(tgt_z=_p(16), kind=3)),
    ('sr3_train_step_ex', dict(kind=3, delta=NAN)), ('sr3_train_step_ex', dict(kind=2, delta=0.0, batch=0)),
    ('sr3_train_step_ex', dict(weight=_p(18), cc=6)), ('sr3_train_step_ex', dict(batch=0, ws_short=1)),
    ('sr3_train_step_ex', dict(ws_short=1, ws=_p(WS, 128))), ('sr3_train_step_ex', dict(ws_short=1, level=None)),
    ('sr3_train_step_ex', dict(params=_p(9, 8), level=None)), ('sr3_train_step_ex', dict(level=None, dropout_p=1.0)),
    ('sr3_train_step_ex', dict(plan='ddpm', tstep=None, dropout_p=1.0)), ('sr3_train_step_ex', dict(plan='var', dropout_p=1.0)),
    ('sr3_train_step_ex2', dict(plan='var', dropout_p=1.0, lam=-1.0)), ('sr3_train_step_ex2', dict(plan='sr3', lam=-1.0)),
    ('sr3_train_step_ex2', dict(plan='var', ws_short=1, lam=-1.0)),
    ('sr3_train_step_ex3', dict(plan='var', dropout_p=1.0, pi_scratch=None)), ('sr3_train_step_ex3', dict(plan='var', pi_scratch=None, lam=-1.0)),
    ('sr3_train_step_ex3', dict(pi_scratch=None, pi_short=1)), ('sr3_train_step_ex3', dict(pi_short=1, pi_out=_p(15))),
    ('sr3_train_step_ex3', dict(pi_out=_p(WS), pi_scratch=_p(WS, 256))), ('sr3_train_step_ex3', dict(pi_out=_p(15), pi_scratch=_p(15, 4))),
    ('sr3_train_step_ex3', dict(pi_out=_p(WS), pi_scratch=_p(15, 4))), ('sr3_train_step_ex3', dict(plan='var', pi_scratch=_p(15, 4), lam=INF)),
    ('sr3_train_step_ex3', dict(plan='var', pi_out=None, pi_scratch=None, lam=-1.0)), ('sr3_train_step_ex3', dict(pi_out=None, pi_scratch=None, dropout_p=1.0)),
]
TWO_LOSS = [
    ('sr3_loss_grad_f32', dict(z=None, kind=3)), ('sr3_loss_grad_f32', dict(kind=3, batch=0)), ('sr3_loss_grad_f32', _tables(hr=None, batch=0)),
    ('sr3_loss_grad_f32', dict(batch=0, channels=5)), ('sr3_loss_grad_f32', dict(channels=5, scratch=_p(9, 4))),
    ('sr3_hybrid_loss_grad_f32', dict(scal=None, kind=3)), ('sr3_hybrid_loss_grad_f32', dict(kind=2, delta=0.0, pixels=0)),
    ('sr3_hybrid_loss_grad_f32', dict(pixels=0, channels=0)), ('sr3_hybrid_loss_grad_f32', dict(channels=5, lam=-1.0)),
    ('sr3_hybrid_loss_grad_f32', dict(lam=NAN, scratch=_p(9, 4))),
]


def _on(entry, rows):
    """(entry, case) of every row; a row that names no plan once per plan the entry serves"""
    out = []
    for kw in rows:
        out += [(entry, kw)] if 'plan' in kw else [(entry, dict(kw, plan=pl)) for pl in ON[entry]]
    return out


def _key(entry, kw):
    """a case as something that compares by value (two ctypes pointers of one address do not)"""
    return entry, sorted((k, v.value if isinstance(v, C.c_void_p) else repr(v)) for k, v in kw.items())


TABLES = {
    'EX': _on('sr3_train_step_ex', COMMON) + [('sr3_train_step_ex', kw) for kw in EX_ONLY],
    'EX2': _on('sr3_train_step_ex2', COMMON) + [('sr3_train_step_ex2', kw) for kw in EX2_ONLY],
    'EX3': _on('sr3_train_step_ex3', COMMON) + [('sr3_train_step_ex3', kw) for kw in EX3_ONLY],
    'LOSS': [('sr3_loss_grad_f32', kw) for kw in LOSS_COMMON + LOSS_ONLY],
    'HYBRID': [('sr3_hybrid_loss_grad_f32', kw) for kw in LOSS_COMMON + HYB_ONLY],
    'TWO_FAULTS': TWO_STEP + TWO_LOSS,
}
CASES = [(t, i) for t in TABLES for i in range(len(TABLES[t]))]


def _call(lib, table, case):
    """-> [return code, the whole message] of one case of one table"""
    entry, kw = TABLES[table][case]
    args = _step_args(entry, **kw) if entry in TAILS else _loss_args(entry, **kw)
    rc = getattr(lib, entry)(*args)
    return [int(rc), lib.sr3_last_error().decode()]


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted('%s[%d]' % c for c in CASES)
    # every refusal the tables are there for is reached by some case of the entry's own table (not met one check early on the wrong plan)
    for table, who, texts in (('EX', 'sr3_train_step_ex', ('go together',)), ('EX2', 'sr3_train_step_ex2', ('step_scalars is NULL', 'go together', 'vlb_lambda -1', 'vlb_lambda inf', 'vlb_lambda nan')),
                              ('EX3', 'sr3_train_step_ex3', ('step_scalars is NULL', 'vlb_lambda -1', 'vlb_lambda inf', 'scratch is NULL', 'scratch too small', 'per_image_out overlaps scratch',
                                                             'overlaps the workspace', 'not 8-byte aligned')),
                              ('HYBRID', 'sr3_hybrid_loss_grad_f32', ('vlb_lambda -1', 'vlb_lambda inf', 'vlb_lambda nan', 'channels 0', 'channels 5', 'batch 0')),
                              ('LOSS', 'sr3_loss_grad_f32', ('hr_nchw is NULL', 'channels 0', 'channels 5', 'batch 0'))):
        got = [recorded['%s[%d]' % (table, i)][1] for i in range(len(TABLES[table]))]
        for text in texts:
            assert any(m.startswith(who + ':') and text in m for m in got), (table, text)
        for text in ('loss_kind', 'huber_delta 0', 'huber_delta nan', 'must be all NULL or all given (1 of 3', 'all given (2 of 3'):
            assert any(m.startswith(who + ':') and text in m for m in got), (table, text)
        if table.startswith('EX'):
            for text in ('null argument', 'workspace too small', 'misaligned pointer', 'needs noise_level', 'needs timestep', 'dropout_p out of range'):
                assert any(text in m for m in got), (table, text)
    assert len(TWO_STEP) + len(TWO_LOSS) >= 8 and {e for e, _ in TABLES['TWO_FAULTS']} == set(TAILS) | {'sr3_loss_grad_f32', 'sr3_hybrid_loss_grad_f32'}


def test_the_order_of_checks_is_the_documented_one(recorded):
    """the fixture itself says what the issue lists: which of two faults each entry reports"""
    def text(entry, **kw):
        return recorded['TWO_FAULTS[%d]' % [_key(*c) for c in TABLES['TWO_FAULTS']].index(_key(entry, kw))][1]
    assert text('sr3_train_step_ex2', plan='var', scal=None, hr=None) == 'sr3_train_step_ex2: step_scalars is NULL'
    assert text('sr3_train_step_ex3', scal=None, hr=None) == 'sr3_train_step_ex3: step_scalars is NULL'
    assert 'loss_kind' in text('sr3_train_step_ex', kind=3, ws_short=1)                         # the objective before build_train and the workspace
    assert 'too small' in text('sr3_train_step_ex', ws_short=1, ws=_p(WS, 128))                 # size before alignment
    assert 'scratch is NULL' in text('sr3_train_step_ex3', plan='var', pi_scratch=None, lam=-1.0)      # the per-image block before vlb_lambda
    assert 'scratch is NULL' in text('sr3_train_step_ex3', pi_scratch=None, pi_short=1)
    assert 'too small' in text('sr3_train_step_ex3', pi_short=1, pi_out=_p(15))
    assert 'per_image_out overlaps scratch' in text('sr3_train_step_ex3', pi_out=_p(15), pi_scratch=_p(15, 4))
    assert 'overlaps the workspace' in text('sr3_train_step_ex3', pi_out=_p(WS), pi_scratch=_p(15, 4))
    assert 'go together' in text('sr3_train_step_ex2', plan='sr3', lam=-1.0)                    # var_channels / step_scalars before vlb_lambda


@pytest.mark.parametrize('table,case', CASES, ids=['%s-%d' % c for c in CASES])
def test_refusal_is_the_recorded_one(recorded, table, case):
    from sr3_hip import lib as L
    got = _call(L.load(), table, case)
    assert got[0] < 0, (table, case, got)      # (a refusal: nothing was launched)
    assert got == recorded['%s[%d]' % (table, case)], (table, case)


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    sys.path[:0] = [root, os.path.join(root, 'image-super-resolution-via-iterative-refinement_amd'), here]
    from sr3_hip import lib as L
    lib = L.load()
    out = {'%s[%d]' % c: _call(lib, *c) for c in CASES}
    bad = [k for k, v in out.items() if v[0] >= 0]
    assert not bad, 'not refused (a launch was attempted): %s' % bad
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d refusals from %s' % (len(out), L.LIB_PATH))
