"""The refusals of the step entries, byte for byte (CPU only: every case refuses before the first launch).

tests/golden/step_refusals.json holds, for every case of the refusal tables of the *_cpu.py tests, of the table for sr3_tiled_step_hist
below and of the two-faults-at-once cases below, the return code and the whole sr3_last_error() text, recorded from the library as it
was before the entries' argument checks moved into csrc/step_tail.h.  Whatever shares those checks has to give the same code and the
same text for the same call, so also the same ORDER of checks: the two-fault cases say which of two faults is reported.

Record again (only from a library whose refusals are the wanted ones):  SR3_LIBRARY=/path/lib.so python tests/test_step_refusals_cpu.py
"""
import ctypes as C
import json
import os
import sys

import pytest

from test_backprojection_cpu import BP_REFUSALS, RESAMPLE_REFUSALS, _bp_args, _host, _resample_args
from test_consistency_cpu import STEP_REFUSALS, _step_args
from test_distill_cpu import D_REFUSALS, T_REFUSALS, _d_args, _t_args
from test_guidance_cpu import G_REFUSALS, Q_REFUSALS, _g_args, _p, _q_args

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_refusals.json')

TS_KEYS = ('x', 'eps', 'batch', 'channels', 'height', 'width', 'oy', 'ny', 'ox', 'nx', 'wy', 'wx', 'th', 'tw', 'oy_host', 'ox_host', 'z', 'ta',
           'tb', 'tc1', 'tc2', 'tsig', 'step2', 'clip', 'eps_out', 'stream', 'c3', 'hist')
TS_IMG = 2 * 3 * 8 * 12 * 4      # bytes of the default image batch


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _ts_args(**kw):
    a = dict(x=_p(1), eps=_p(2), batch=2, channels=3, height=8, width=12, oy=_p(3), ny=2, ox=_p(4), nx=2, wy=_p(5), wx=_p(6), th=4, tw=8,
             oy_host=_ints(0, 4), ox_host=_ints(0, 4), z=None, ta=_p(7), tb=_p(8), tc1=_p(9), tc2=_p(10), tsig=_p(11), step2=_p(12), clip=1,
             eps_out=None, stream=None, c3=None, hist=None)
    a.update(kw)
    return [a[k] for k in TS_KEYS]


HUGE = dict(batch=1 << 12, channels=2, height=1 << 9, width=1 << 9)      # 2^31 elements

# sr3_tiled_step_hist: (arguments, code, a word of the message); the fixture pins the whole text
TS_REFUSALS = [
    (dict(x=None), -1, 'null'), (dict(eps=None), -1, 'null'), (dict(oy=None), -1, 'null'), (dict(wx=None), -1, 'null'), (dict(ta=None), -1, 'null'),
    (dict(tsig=None), -1, 'null'), (dict(step2=None), -1, 'null'),
    (dict(batch=0), -1, 'positive'), (dict(width=-12), -1, 'positive'), (dict(ny=0), -1, 'positive'), (dict(tw=0), -1, 'positive'),
    (dict(th=16), -1, 'larger than the image'), (dict(tw=16), -1, 'larger than the image'),
    (dict(HUGE, oy_host=None, ox_host=None), -2, '2^31'), (dict(ny=1 << 15, nx=1 << 15, oy_host=None, ox_host=None), -2, '2^31'),
    (dict(oy_host=_ints(1, 4)), -1, 'y origins must start'), (dict(ox_host=_ints(0, 3)), -1, 'x origins must start'),
    (dict(nx=3, ox_host=_ints(0, 4, 4)), -1, 'not strictly increasing'), (dict(height=16, oy_host=_ints(0, 12)), -1, 'leave a gap'),
    (dict(c3=_p(13)), -1, 'c3'), (dict(hist=_p(14)), -1, 'c3'),
    (dict(c3=_p(13), hist=_p(1)), -1, 'history overlaps'), (dict(c3=_p(13), hist=_p(1, TS_IMG - 4)), -1, 'history overlaps'),
    (dict(c3=_p(13), hist=_p(15), eps_out=_p(15, 16)), -1, 'history overlaps'),
    (dict(x=_p(1, 4)), -3, 'misaligned'), (dict(z=_p(16, 8)), -3, 'misaligned'), (dict(eps_out=_p(16, 4)), -3, 'misaligned'),
    (dict(c3=_p(13), hist=_p(14, 4)), -3, 'misaligned'),
]

ENTRIES = {
    'STEP_REFUSALS': ('sr3_consistent_step', _step_args, STEP_REFUSALS),
    'G_REFUSALS': ('sr3_guided_step', _g_args, G_REFUSALS),
    'Q_REFUSALS': ('sr3_abs_quantile_f32', _q_args, Q_REFUSALS),
    'BP_REFUSALS': ('sr3_backproject_step', _bp_args, BP_REFUSALS),
    'RESAMPLE_REFUSALS': ('sr3_resample_f32', _resample_args, RESAMPLE_REFUSALS),
    'T_REFUSALS': ('sr3_teacher_step_f32', _t_args, T_REFUSALS),
    'D_REFUSALS': ('sr3_distill_target_f32', _d_args, D_REFUSALS),
    'TS_REFUSALS': ('sr3_tiled_step_hist', _ts_args, TS_REFUSALS),
}

# two faults in one call, per entry: the one reported is the one the checks meet first
ENTRIES['TWO_FAULTS'] = (None, None, [
    ('STEP_REFUSALS', dict(x=None, batch=0)), ('STEP_REFUSALS', dict(HUGE, block=3)), ('STEP_REFUSALS', dict(HUGE, height=(1 << 9) + 2)),
    ('STEP_REFUSALS', dict(strength=float('nan'), c3=_p(10))), ('STEP_REFUSALS', dict(c3=_p(10), y=_p(1))), ('STEP_REFUSALS', dict(step2=None, block=3)),
    ('G_REFUSALS', dict(step2=None, width=0)), ('G_REFUSALS', dict(HUGE, mode=3)), ('G_REFUSALS', dict(mode=3, scale=float('nan'))),
    ('G_REFUSALS', dict(scale=float('inf'), x0=None)), ('G_REFUSALS', dict(x0=None, rank_lo=-1)), ('G_REFUSALS', dict(qs=None, c3=_p(10))),
    ('G_REFUSALS', dict(hist=_p(11), x0=_p(1))), ('G_REFUSALS', dict(x0=_p(1), out_u=_p(1))), ('G_REFUSALS', dict(out_u=_p(2), thr=_p(2))),
    ('G_REFUSALS', dict(c3=_p(10), hist=_p(12), z=_p(1))), ('G_REFUSALS', dict(step2=_p(1), thr=_p(3))),
    ('Q_REFUSALS', dict(src=None, batch=0)), ('Q_REFUSALS', dict(batch=1 << 12, n=1 << 19, rank_lo=-1)), ('Q_REFUSALS', dict(frac=1.0, scratch=None)),
    ('BP_REFUSALS', dict(uwv=None, batch=0)), ('BP_REFUSALS', dict(HUGE, scale=3)), ('BP_REFUSALS', dict(HUGE, scale=1)),
    ('BP_REFUSALS', dict(HUGE, iterations=0)), ('BP_REFUSALS', dict(iterations=0, strength=float('nan'))), ('BP_REFUSALS', dict(strength=2.0, ukv=0)),
    ('BP_REFUSALS', dict(dkh=0, c3=_p(18))), ('BP_REFUSALS', dict(hist=_p(19), scratch=None)), ('BP_REFUSALS', dict(scratch_bytes=0, y=_p(1))),
    ('BP_REFUSALS', dict(y=_p(1), scratch=_p(2))), ('BP_REFUSALS', dict(c3=_p(18), hist=_p(3), scratch=_p(9))),
    ('RESAMPLE_REFUSALS', dict(tmp=None, planes=0)), ('RESAMPLE_REFUSALS', dict(kh=0, kv=0)), ('RESAMPLE_REFUSALS', dict(dst=_p(1), tmp=_p(1))),
    ('RESAMPLE_REFUSALS', dict(tmp=_p(5), bh_host=_host([(0, 8), (0, 12), (-1, 4)]))),
    ('T_REFUSALS', dict(x0_out=None, batch=0)), ('T_REFUSALS', dict(batch=1 << 12, per=1 << 19, scale=float('nan'))), ('T_REFUSALS', dict(per=0, scale=float('nan'))),
    ('T_REFUSALS', dict(scale=float('inf'), x_next=_p(2))), ('T_REFUSALS', dict(x_next=_p(1, 4), x0_out=_p(1))), ('T_REFUSALS', dict(x_next=_p(2), x0_out=_p(2))),
    ('T_REFUSALS', dict(x_next=_p(1), x0_out=_p(3))), ('T_REFUSALS', dict(out_u=None, scale=float('nan'), x_next=_p(7))),
    ('D_REFUSALS', dict(eps_tgt=None, per=0)), ('D_REFUSALS', dict(batch=1 << 12, per=1 << 19, scale=float('nan'))), ('D_REFUSALS', dict(scale=float('nan'), x_tgt=_p(1))),
    ('D_REFUSALS', dict(x_tgt=_p(2), eps_tgt=_p(1))), ('D_REFUSALS', dict(x_tgt=_p(11), eps_tgt=_p(11))), ('D_REFUSALS', dict(x_tgt=_p(2), z_t=_p(13))),
    ('TS_REFUSALS', dict(step2=None, batch=0)), ('TS_REFUSALS', dict(HUGE, th=1 << 10)), ('TS_REFUSALS', dict(ny=0, th=16)),
    ('TS_REFUSALS', dict(HUGE, oy_host=_ints(1, 4))), ('TS_REFUSALS', dict(oy_host=_ints(1, 4), ox_host=_ints(0, 3))), ('TS_REFUSALS', dict(ox_host=_ints(0, 3), c3=_p(13))),
    ('TS_REFUSALS', dict(hist=_p(14), x=_p(1, 4))), ('TS_REFUSALS', dict(c3=_p(13), hist=_p(1, 4))), ('TS_REFUSALS', dict(width=10, tw=5, ox_host=_ints(0, 5), x=_p(1, 4), c3=_p(13))),
])


def _call(lib, table, case):
    """-> [return code, the whole message] of one case of one table"""
    entry, build, rows = ENTRIES[table]
    if table == 'TWO_FAULTS':
        base, kw = rows[case]
        entry, build, _ = ENTRIES[base]
    else:
        kw = rows[case][0]
    rc = getattr(lib, entry)(*build(**kw))
    return [int(rc), lib.sr3_last_error().decode()]


CASES = [(t, i) for t in ENTRIES for i in range(len(ENTRIES[t][2]))]


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted('%s[%d]' % c for c in CASES)
    assert len(TS_REFUSALS) >= 12 and {ENTRIES['TWO_FAULTS'][2][i][0] for i in range(len(ENTRIES['TWO_FAULTS'][2]))} == set(ENTRIES) - {'TWO_FAULTS'}


@pytest.mark.parametrize('table,case', CASES, ids=['%s-%d' % c for c in CASES])
def test_refusal_is_the_recorded_one(recorded, table, case):
    from sr3_hip import lib as L
    got = _call(L.load(), table, case)
    assert got[0] < 0, (table, case, got)      # (a refusal: nothing was launched)
    assert got == recorded['%s[%d]' % (table, case)], (table, case)


@pytest.mark.parametrize('case', range(len(TS_REFUSALS)))
def test_tiled_step_refusals_no_gpu(case):
    """every refusal of sr3_tiled_step_hist returns its code and says what is wrong, before any launch: no device is present here"""
    from sr3_hip import lib as L
    lib = L.load()
    kw, code, word = TS_REFUSALS[case]
    assert lib.sr3_tiled_step_hist(*_ts_args(**kw)) == code, kw
    msg = lib.sr3_last_error().decode()
    assert word in msg and (msg.startswith('tiled_step') or msg.startswith('tiling') or code == -3), (kw, msg)


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
