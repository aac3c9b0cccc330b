"""The refusals of the per-op entries of the training backward (sr3_groupnorm_act_bwd_f32, sr3_conv_dgrad_f32, sr3_grad_route_f32,
sr3_colsums_f32, sr3_embed_bwd_f32), CPU only: every case must return its code and name what is wrong before anything is launched --
no device is present here, and every pointer is a made-up address that no case may touch."""
import ctypes as C

import pytest

NOMEM, ALIGN, UNSUP, BADARG = -4, -3, -2, -1


def _p(k, off=0):
    """a made-up, 256-byte aligned, non-NULL address: every case refuses before it touches memory"""
    return C.c_void_p((k << 24) + off)


def _plan():
    from sr3_hip import engine as E
    return E.Plan('sr3', 6, 3, 8, 4, [1, 2], [8], 1, 16)


GN_KEYS = ('dA', 'x0', 'C0', 'x1', 'C1', 'B', 'HW', 'ss', 'mr', 'groups', 'act', 'gamma', 'seed', 'p', 'dgamma', 'dbeta', 'dx0', 'acc0',
           'dx1', 'acc1', 'aout', 'scratch', 'scratch_bytes', 'stream')


def _gn_args(**kw):
    a = dict(dA=_p(1), x0=_p(2), C0=8, x1=_p(3), C1=16, B=2, HW=35, ss=_p(4), mr=_p(5), groups=4, act=2, gamma=_p(6), seed=7, p=0.0,
             dgamma=_p(7), dbeta=_p(8), dx0=_p(9), acc0=0, dx1=_p(10), acc1=1, aout=None, scratch=_p(11), scratch_bytes=1 << 20, stream=None)
    a.update(kw)
    return [a[k] for k in GN_KEYS]


GN_REFUSALS = [
    (dict(dA=None), BADARG, 'NULL'), (dict(x0=None), BADARG, 'NULL'), (dict(ss=None), BADARG, 'NULL'), (dict(mr=None), BADARG, 'NULL'),
    (dict(gamma=None), BADARG, 'NULL'), (dict(dgamma=None), BADARG, 'NULL'), (dict(dbeta=None), BADARG, 'NULL'), (dict(dx0=None), BADARG, 'NULL'),
    (dict(dx1=None), BADARG, 'NULL'), (dict(x1=None), BADARG, 'NULL'), (dict(scratch=None), BADARG, 'NULL'),
    (dict(B=0), BADARG, 'positive'), (dict(HW=-1), BADARG, 'positive'), (dict(groups=0), BADARG, 'positive'),
    (dict(C0=6), UNSUP, 'multiples of 4'), (dict(C1=10), UNSUP, 'multiples of 4'),
    (dict(groups=5), UNSUP, 'do not divide'), (dict(x1=None, dx1=None, C1=0, groups=3), UNSUP, 'do not divide'),
    (dict(act=0), BADARG, 'act'), (dict(act=3), BADARG, 'act'), (dict(p=1.0), BADARG, 'drop_p'), (dict(p=-0.1), BADARG, 'drop_p'),
    (dict(p=float('nan')), BADARG, 'drop_p'),
    (dict(scratch=_p(11, 4)), ALIGN, 'aligned'), (dict(scratch_bytes=0), NOMEM, 'scratch too small'),
    (dict(B=1 << 12, HW=1 << 16, C0=8, C1=0), UNSUP, '2^31'),
]

DG_KEYS = ('plan', 'dy', 'w', 'Cout_w', 'CoutP', 'B', 'Hs', 'Ws', 'ups', 'stride', 'ksize', 'Cin', 'dA', 'scratch', 'scratch_bytes', 'derived',
           'derived_bytes', 'tile', 'ksplit', 'kind', 'stream')


def _dg_args(the_plan, **kw):
    a = dict(plan=the_plan.handle, dy=_p(1), w=_p(2), Cout_w=32, CoutP=32, B=1, Hs=16, Ws=16, ups=0, stride=1, ksize=3, Cin=32, dA=_p(3),
             scratch=_p(4), scratch_bytes=1 << 24, derived=_p(5), derived_bytes=1 << 24, tile=None, ksplit=None, kind=None, stream=None)
    a.update(kw)
    return [a[k] for k in DG_KEYS]


DG_REFUSALS = [
    (dict(plan=None), BADARG, 'NULL'), (dict(dy=None), BADARG, 'NULL'), (dict(w=None), BADARG, 'NULL'), (dict(dA=None), BADARG, 'NULL'),
    (dict(scratch=None), BADARG, 'NULL'),
    (dict(B=0), BADARG, 'positive'), (dict(Ws=0), BADARG, 'positive'), (dict(Cin=0), BADARG, 'positive'),
    (dict(Cin=30), UNSUP, 'multiples of 4'), (dict(CoutP=6, Cout_w=6), UNSUP, 'multiples of 4'),
    (dict(Cout_w=0), BADARG, 'Cout_w'), (dict(Cout_w=33), BADARG, 'Cout_w'),
    (dict(stride=2, Hs=15), UNSUP, 'even input map'), (dict(stride=2, Ws=7), UNSUP, 'even input map'),
    (dict(stride=3), BADARG, 'out of range'), (dict(ksize=5), BADARG, 'out of range'), (dict(ups=2), BADARG, 'out of range'),
    (dict(ups=1, stride=2), UNSUP, 'unsupported'),
    (dict(scratch=_p(4, 16)), ALIGN, 'aligned'), (dict(derived=_p(5, 64)), ALIGN, 'aligned'),
    (dict(scratch_bytes=0), NOMEM, 'scratch too small'), (dict(scratch_bytes=1024), NOMEM, 'scratch too small'),
    # room for the filters and nothing else: the general kernel's split-K slabs of this 8 x 8 map do not fit
    (dict(B=1, Hs=8, Ws=8, Cin=128, CoutP=128, Cout_w=128, ksize=3, derived=None, derived_bytes=0, scratch_bytes=128 * 9 * 128 * 4), NOMEM,
     'scratch too small'),
    (dict(B=1 << 10, Hs=1 << 9, Ws=1 << 9, Cin=8, CoutP=8, Cout_w=8), UNSUP, '2^31'),
]

GR_KEYS = ('g', 'C0', 'C1', 'B', 'Hs', 'Ws', 'ups', 'd0', 'acc0', 'd1', 'acc1', 'stream')


def _gr_args(**kw):
    a = dict(g=_p(1), C0=8, C1=16, B=2, Hs=5, Ws=7, ups=1, d0=_p(2), acc0=0, d1=_p(3), acc1=1, stream=None)
    a.update(kw)
    return [a[k] for k in GR_KEYS]


GR_REFUSALS = [
    (dict(g=None), BADARG, 'NULL'), (dict(d0=None), BADARG, 'NULL'), (dict(d1=None), BADARG, 'NULL'),
    (dict(B=0), BADARG, 'positive'), (dict(Hs=0), BADARG, 'positive'), (dict(C0=0), BADARG, 'positive'), (dict(C1=-4), BADARG, 'positive'),
    (dict(ups=2), BADARG, 'ups'), (dict(C0=6), UNSUP, 'multiples of 4'), (dict(C1=2), UNSUP, 'multiples of 4'),
    (dict(B=1 << 10, Hs=1 << 9, Ws=1 << 9, ups=0), UNSUP, '2^31'),
]

CS_KEYS = ('g', 'B', 'HW', 'C', 'dbias', 'dfilm', 'film_stride', 'scratch', 'scratch_bytes', 'stream')


def _cs_args(**kw):
    a = dict(g=_p(1), B=3, HW=35, C=8, dbias=_p(2), dfilm=_p(3), film_stride=40, scratch=_p(4), scratch_bytes=1 << 20, stream=None)
    a.update(kw)
    return [a[k] for k in CS_KEYS]


CS_REFUSALS = [
    (dict(g=None), BADARG, 'NULL'), (dict(scratch=None), BADARG, 'NULL'), (dict(dbias=None, dfilm=None), BADARG, 'NULL'),
    (dict(B=0), BADARG, 'positive'), (dict(HW=0), BADARG, 'positive'), (dict(C=0), BADARG, 'positive'),
    (dict(C=6), UNSUP, 'multiple of 4'), (dict(film_stride=4), BADARG, 'film_stride'),
    (dict(scratch=_p(4, 4)), ALIGN, 'aligned'), (dict(scratch_bytes=8), NOMEM, 'scratch too small'),
    (dict(B=1 << 12, HW=1 << 16), UNSUP, '2^31'),
]

EB_KEYS = ('variant', 'B', 'inner', 'F', 'level', 'tstep', 'freq', 'w1', 'b1', 'w2', 'b2', 'wf', 'dfilm', 'dw1', 'db1', 'dw2', 'db2', 'dwf', 'dbf',
           'scratch', 'scratch_bytes', 'stream')


def _eb_args(**kw):
    a = dict(variant=0, B=2, inner=8, F=40, level=_p(1), tstep=None, freq=_p(2), w1=_p(3), b1=_p(4), w2=_p(5), b2=_p(6), wf=_p(7), dfilm=_p(8),
             dw1=_p(9), db1=_p(10), dw2=_p(11), db2=_p(12), dwf=_p(13), dbf=_p(14), scratch=_p(15), scratch_bytes=1 << 20, stream=None)
    a.update(kw)
    return [a[k] for k in EB_KEYS]


EB_REFUSALS = [
    (dict(freq=None), BADARG, 'NULL'), (dict(w1=None), BADARG, 'NULL'), (dict(wf=None), BADARG, 'NULL'), (dict(dfilm=None), BADARG, 'NULL'),
    (dict(dw1=None), BADARG, 'NULL'), (dict(dbf=None), BADARG, 'NULL'), (dict(scratch=None), BADARG, 'NULL'),
    (dict(level=None), BADARG, 'noise level'), (dict(variant=1), BADARG, 'timestep'), (dict(variant=2), BADARG, 'variant'),
    (dict(B=0), BADARG, 'positive'), (dict(F=0), BADARG, 'positive'), (dict(inner=1), BADARG, 'positive'),
    (dict(inner=24), UNSUP, 'inner must divide 256'), (dict(inner=96), UNSUP, 'inner must divide 256'), (dict(inner=512), UNSUP, 'inner must divide 256'),
    (dict(scratch=_p(15, 2)), ALIGN, 'aligned'), (dict(scratch_bytes=2 * 29 * 8 * 4 - 4), NOMEM, 'scratch too small'),
]

TABLES = {
    'sr3_groupnorm_act_bwd_f32': (_gn_args, GN_REFUSALS, False),
    'sr3_conv_dgrad_f32': (_dg_args, DG_REFUSALS, True),
    'sr3_grad_route_f32': (_gr_args, GR_REFUSALS, False),
    'sr3_colsums_f32': (_cs_args, CS_REFUSALS, False),
    'sr3_embed_bwd_f32': (_eb_args, EB_REFUSALS, False),
}
CASES = [(e, i) for e in TABLES for i in range(len(TABLES[e][1]))]


@pytest.mark.parametrize('entry,case', CASES, ids=['%s-%d' % (e[4:-4], i) for e, i in CASES])
def test_refusal_before_any_launch(entry, case):
    from sr3_hip import lib as L
    lib = L.load()
    build, rows, wants_plan = TABLES[entry]
    kw, code, word = rows[case]
    plan = _plan() if wants_plan else None
    args = build(plan, **kw) if wants_plan else build(**kw)
    assert getattr(lib, entry)(*args) == code, kw
    msg = lib.sr3_last_error().decode()
    assert word in msg, (kw, msg)
    # the message names the entry, or (the one refusal that predates the entries) the function the step calls
    assert msg.startswith(entry) or msg.startswith('embed_backward'), msg


def test_scratch_queries():
    """the byte counts the entries check against: 0 for a shape the entry refuses, the step's own sizes otherwise"""
    from sr3_hip import lib as L
    lib = L.load()
    assert lib.sr3_groupnorm_act_bwd_scratch_bytes(2, 35, 24, 5) == 0 and lib.sr3_groupnorm_act_bwd_scratch_bytes(2, 35, 22, 2) == 0
    T = lib.sr3_groupnorm_stats_slices(2, 35, 24)
    part = 2 * T * 24 * 2 * 8
    assert lib.sr3_groupnorm_act_bwd_scratch_bytes(2, 35, 24, 4) == (part + 255) // 256 * 256 + 2 * 4 * 2 * 8
    assert lib.sr3_colsums_scratch_bytes(3, 35, 6) == 0 and lib.sr3_colsums_scratch_bytes(0, 35, 8) == 0
    assert lib.sr3_colsums_scratch_bytes(3, 35, 8) == 3 * lib.sr3_groupnorm_stats_slices(3, 35, 8) * 8 * 2 * 8
    assert lib.sr3_embed_bwd_scratch_bytes(3, 64) == 3 * 29 * 64 * 4 and lib.sr3_embed_bwd_scratch_bytes(0, 64) == 0
    plan = _plan()
    nd, base = C.c_size_t(123), C.c_size_t(123)
    assert lib.sr3_conv_dgrad_scratch_bytes(plan.handle, 1, 15, 16, 0, 2, 3, 16, 16, C.byref(nd), C.byref(base)) == 0
    assert nd.value == 0 and base.value == 0
    # a 16 x 16 map on the default plan: the one-image Winograd tile reads its 3 x bf16 split filters from `derived`
    nb = lib.sr3_conv_dgrad_scratch_bytes(plan.handle, 1, 16, 16, 0, 1, 3, 32, 32, C.byref(nd), C.byref(base))
    assert nb >= base.value == 32 * 9 * 32 * 4 and nd.value > 32 * 9 * 32 * 4
    # stride 2: the zero-inserted dy sits between the filters and the slabs
    assert lib.sr3_conv_dgrad_scratch_bytes(plan.handle, 2, 16, 24, 0, 2, 3, 16, 16, None, C.byref(base)) >= base.value == 16 * 9 * 16 * 4 + 2 * 16 * 24 * 16 * 4
    plan.set_option('winograd', 0)
    assert lib.sr3_conv_dgrad_scratch_bytes(plan.handle, 1, 16, 16, 0, 1, 3, 32, 32, C.byref(nd), None) > 0 and nd.value == 0


def test_signatures_match_the_header():
    import os
    import re
    from helpers import ROOT
    from sr3_hip import lib as L
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sr3_mi355x.h')).read(), flags=re.S)
    lib = L.load()
    for name in list(TABLES) + ['sr3_groupnorm_act_bwd_scratch_bytes', 'sr3_conv_dgrad_scratch_bytes', 'sr3_colsums_scratch_bytes',
                                'sr3_embed_bwd_scratch_bytes', 'sr3_groupnorm_fold_mr_f32']:
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, src).group(1)
        assert len(L.SIGNATURES[name][1]) == decl.count(',') + 1, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
