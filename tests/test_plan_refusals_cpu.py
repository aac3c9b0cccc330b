"""The refusals of the plan's entries, byte for byte, and what setting an option does to a plan that has already built its launch lists
(CPU only: every case returns before the first HIP call).

tests/golden/plan_refusals.json holds, for every case of the tables below, the return code and the whole sr3_last_error() text, recorded
from the library as it was while csrc/plan.hip wrote the front checks out in each of unet_forward_rows, sr3_reverse_step_hist and
sr3_unet_forward_profile and sr3_plan_set_option was a strcmp chain.  Whatever shares those checks has to give the same code and the same
text for the same call, so also the same ORDER of checks: the two-fault cases say which of two faults is reported.  Every case is called
with the error text set to 'bad param index' first, so a refusal that leaves the text alone (a null plan or key at sr3_plan_set_option)
records exactly that.

Only the pointers an entry checks are cases: sr3_unet_forward_profile checks neither x / params / eps / freq nor any alignment, the
other entries check no alignment of cond, freq or the tables -- such a call reaches the first launch, which is not a refusal.

Record again (only from a library whose refusals are the wanted ones):  SR3_LIBRARY=/path/lib.so python tests/test_plan_refusals_cpu.py
"""
import ctypes as C
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'plan_refusals.json')
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'sr3_mi355x.h')
B = 2
NETS = ('sr3_tiny', 'ddpm_tiny')
BADARG = -1


def _p(k, off=0):
    """a made-up, 256-byte aligned, non-NULL address: every case refuses before it touches memory"""
    return C.c_void_p((k << 24) + off)


WS = 64                      # the workspace's address number: the highest one, so that nothing lies behind it whatever its size
_plans = {}


def _fresh(net, **kw):
    from helpers import DESCS
    from sr3_hip import engine as E
    d = dict(DESCS[net], **kw)
    return E.Plan(d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'], d['attn_res'],
                  d['res_blocks'], d['image_size'])


def _plan(net):
    """-> (the plan every forward / step case of `net` shares, its workspace bytes at batch B): no case changes it, each refuses"""
    if net not in _plans:
        plan = _fresh(net)
        _plans[net] = (plan, plan.workspace_bytes(B))
    return _plans[net]


FWD_KEYS = ('x', 'cond', 'cc', 'level', 'tstep', 'freq', 'level_table', 'step_dev', 'params', 'ws', 'ws_bytes', 'eps', 'batch', 'stream')
STEP_KEYS = ('x', 'cond', 'cc', 'freq', 'level_table', 'step2', 'params', 'ws', 'ws_bytes', 'z', 'ta', 'tb', 'tc1', 'tc2', 'tsig', 'clip', 'eps',
             'batch', 'stream')
PROF_KEYS = ('x', 'cond', 'cc', 'level', 'tstep', 'freq', 'params', 'ws', 'ws_bytes', 'eps', 'batch', 'stream', 'max_ops', 'op_ms', 'op_kind',
             'op_flops', 'n_ops')
ENTRY_KEYS = {
    'sr3_unet_forward': FWD_KEYS, 'sr3_unet_forward_full': FWD_KEYS + ('t_map',),
    'sr3_reverse_step': STEP_KEYS, 'sr3_reverse_step_ex': STEP_KEYS + ('t_map',), 'sr3_reverse_step_hist': STEP_KEYS + ('t_map', 'c3', 'hist'),
    'sr3_unet_forward_profile': PROF_KEYS,
}
IMG = B * 3 * 16 * 16 * 4      # bytes of x / eps / hist of a step


def _run_args(entry, net, ws_short=0, no_plan=False, **kw):
    """the arguments of one forward / step / profile entry on the plan of `net`: a call that would run, then `kw`"""
    plan, need = _plan(net)
    ddpm = net == 'ddpm_tiny'
    a = dict(x=_p(1), cond=None if ddpm else _p(2), cc=0 if ddpm else 3, level=None if ddpm else _p(3), tstep=_p(4) if ddpm else None, freq=_p(5),
             level_table=_p(6), step_dev=None, step2=_p(7), params=_p(8), ws=_p(WS), ws_bytes=need - ws_short, eps=_p(9), batch=B, stream=None,
             t_map=None, z=_p(10), ta=_p(11), tb=_p(12), tc1=_p(13), tc2=_p(14), tsig=_p(15), clip=1, c3=None, hist=None,
             max_ops=4096, op_ms=_p(16), op_kind=_p(17), op_flops=_p(18), n_ops=_p(19))
    a.update(kw)
    return [None if no_plan else plan.handle] + [a[k] for k in ENTRY_KEYS[entry]]


# what sr3_unet_forward and sr3_unet_forward_full refuse, on either network ...
FWD = [dict(no_plan=True)] + [{k: None} for k in ('x', 'params', 'ws', 'eps', 'freq')] + [
    dict(batch=0), dict(batch=-3), dict(cond=_p(2), cc=-1), dict(cond=_p(2), cc=6), dict(cond=_p(2), cc=3, net='ddpm_tiny'), dict(ws_short=1),
    dict(ws=_p(WS, 4)), dict(params=_p(8, 4)), dict(x=_p(1, 4)), dict(eps=_p(9, 4)),
    dict(level=None, net='sr3_tiny'), dict(tstep=None, net='ddpm_tiny'),
    # two faults: the one reported is the one the checks meet first
    dict(x=None, batch=0), dict(batch=0, ws_short=1), dict(cond=_p(2), cc=-1, ws=_p(WS, 4)), dict(ws_short=1, ws=_p(WS, 4)), dict(ws_short=1, level=None, tstep=None),
    dict(x=_p(1, 4), level=None, tstep=None),
]
FULL_ONLY = [dict(t_map=_p(20)), dict(t_map=_p(20), x=None), dict(t_map=_p(20), batch=0)]
# ... the three reverse-step entries ...
STEP = [dict(no_plan=True)] + [{k: None} for k in ('x', 'params', 'ws', 'freq', 'step2', 'ta', 'tb', 'tc1', 'tc2', 'tsig')] + [
    dict(batch=0), dict(cond=_p(2), cc=-1), dict(cond=_p(2), cc=6), dict(ws_short=1),
    dict(ws=_p(WS, 4)), dict(params=_p(8, 4)), dict(x=_p(1, 4)), dict(eps=_p(9, 4)), dict(z=_p(10, 4)),
    dict(level_table=None, net='sr3_tiny'),
    dict(ta=None, batch=0), dict(batch=0, ws_short=1), dict(ws_short=1, z=_p(10, 4)), dict(z=_p(10, 4), level_table=None, net='sr3_tiny'),
]
HIST_ONLY = [dict(c3=_p(21)), dict(hist=_p(22)), dict(c3=_p(21), hist=_p(1)), dict(c3=_p(21), hist=_p(1, IMG - 4)), dict(c3=_p(21), hist=_p(9, 16)),
             dict(c3=_p(21), hist=_p(22, 4)),
             dict(level_table=None, c3=_p(21), net='sr3_tiny'), dict(z=_p(10, 4), hist=_p(22)), dict(ws_short=1, c3=_p(21))]
# ... and sr3_unet_forward_profile (it checks no alignment and none of x / params / eps / freq)
PROFILE = [dict(no_plan=True)] + [{k: None} for k in ('op_ms', 'op_kind', 'op_flops', 'n_ops')] + [
    dict(batch=0), dict(cond=_p(2), cc=-1), dict(cond=_p(2), cc=6), dict(ws_short=1), dict(op_ms=None, batch=0), dict(batch=0, ws_short=1)]


def _on(entry, rows):
    """(entry, net, case) of every row; a row that names no network once per network"""
    out = []
    for kw in rows:
        kw = dict(kw)
        nets = (kw.pop('net'),) if 'net' in kw else NETS
        out += [(entry, net, kw) for net in nets]
    return out


# sr3_plan_set_option: (options set first, key, value); every case on a plan of its own
OPTION = [
    ([], 'store_wt', -1), ([], 'store_wt', 8), ([], 'gemm_epi', -1), ([], 'gemm_epi', 3), ([], 'var_channels', 1), ([], 'var_channels', 3),
    ([], 'attn_heads', 0), ([], 'attn_heads', -2), ([], 'attn_heads', 3), ([], 'attn_heads', 8), ([], 'attn_heads', 32),
    ([], 'attn_head_dim', -1), ([], 'attn_head_dim', 2), ([], 'attn_head_dim', 6), ([], 'attn_head_dim', 32),
    ([('attn_heads', 2)], 'attn_head_dim', 4), ([('attn_head_dim', 4)], 'attn_heads', 2), ([('attn_heads', 2)], 'attn_head_dim', -1),
    ([], 'nonsense', 1), ([], '', 0), ([], 'Winograd', 0), ([], 'fuse_stats ', 0), ([], None, 1), ([], 'split_bf16', 1),
]
GEOMETRY = [(17, 16), (16, 17), (17, 17), (-16, 16), (0, 16), (16, 0), (1, 1)]      # (sr3_tiny halves twice: 18 x 16, a multiple of 2, below)
DERIVED = ['bind_null_plan', 'bind_short', 'bind_misaligned', 'bind_short_and_misaligned', 'prepare_null_plan', 'prepare_null_params', 'prepare_unbound']

TABLES = {
    'FORWARD': _on('sr3_unet_forward', FWD),
    'FORWARD_FULL': _on('sr3_unet_forward_full', FWD + FULL_ONLY),
    'STEP': _on('sr3_reverse_step', STEP),
    'STEP_EX': _on('sr3_reverse_step_ex', STEP),
    'STEP_HIST': _on('sr3_reverse_step_hist', STEP + HIST_ONLY),
    'PROFILE': _on('sr3_unet_forward_profile', PROFILE),
    'OPTION': [('sr3_plan_set_option', net, row) for net in NETS for row in OPTION] + [('sr3_plan_set_option', None, ([], 'winograd', 0))],
    'GEOMETRY': [('sr3_plan_set_geometry', net, g) for net in NETS for g in GEOMETRY] + [('sr3_plan_set_geometry', 'sr3_tiny', (18, 16)), ('sr3_plan_set_geometry', 'sr3_tiny', (16, 24 + 2)),
                                                                                                  ('sr3_plan_set_geometry', None, (16, 16))],
    'DERIVED': [('derived', net, what) for net in NETS for what in DERIVED],
}
CASES = [(t, i) for t in TABLES for i in range(len(TABLES[t]))]


def _call(lib, table, case):
    """-> [return code, the whole message] of one case of one table"""
    entry, net, row = TABLES[table][case]
    assert lib.sr3_plan_param_info(None, 0, None) == BADARG and lib.sr3_last_error() == b'bad param index'
    if table == 'OPTION':
        before, key, value = row
        plan = _fresh(net) if net else None
        for k, v in before:
            plan.set_option(k, v)
        assert not before or lib.sr3_plan_param_info(None, 0, None) == BADARG
        rc = lib.sr3_plan_set_option(plan.handle if plan else None, key.encode() if key is not None else None, value)
    elif table == 'GEOMETRY':
        plan = _fresh(net) if net else None
        rc = lib.sr3_plan_set_geometry(plan.handle if plan else None, *row)
    elif table == 'DERIVED':
        plan = _fresh(net)
        need = int(lib.sr3_plan_derived_bytes(plan.handle))
        assert need > 16
        rc = {'bind_null_plan': lambda: lib.sr3_plan_bind_derived(None, _p(1), need),
              'bind_short': lambda: lib.sr3_plan_bind_derived(plan.handle, _p(1), need - 1),
              'bind_misaligned': lambda: lib.sr3_plan_bind_derived(plan.handle, _p(1, 8), need),
              'bind_short_and_misaligned': lambda: lib.sr3_plan_bind_derived(plan.handle, _p(1, 8), need - 1),
              'prepare_null_plan': lambda: lib.sr3_plan_prepare_derived(None, _p(2), None),
              'prepare_null_params': lambda: lib.sr3_plan_prepare_derived(plan.handle, None, None),
              'prepare_unbound': lambda: lib.sr3_plan_prepare_derived(plan.handle, _p(2), None)}[row]()
    else:
        rc = getattr(lib, entry)(*_run_args(entry, net, **row))
    return [int(rc), lib.sr3_last_error().decode()]


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted('%s[%d]' % c for c in CASES)
    texts = {t: [recorded['%s[%d]' % (t, i)][1] for i in range(len(TABLES[t]))] for t in TABLES}
    # every refusal the tables are there for is reached by some case of the entry's own table
    for t in ('FORWARD', 'FORWARD_FULL', 'STEP', 'STEP_EX', 'STEP_HIST', 'PROFILE'):
        for word in ('null argument', 'batch must be > 0', 'cond_channels -1 out of range', 'cond_channels 6 out of range', 'workspace too small'):
            assert any(word in m for m in texts[t]), (t, word)
    for t in ('FORWARD', 'FORWARD_FULL', 'STEP', 'STEP_EX', 'STEP_HIST'):
        assert any(m == 'misaligned pointer (workspace 256 B, tensors 16 B)' for m in texts[t]), t
        assert any(re.fullmatch(r'workspace too small: \d+ < \d+', m) for m in texts[t]), t
    assert 'workspace too small' in texts['PROFILE'] and not any('misaligned' in m for m in texts['PROFILE'])
    for t in ('FORWARD', 'FORWARD_FULL'):
        assert 'SR3 variant needs noise_level or step_dev' in texts[t] and 'DDPM variant needs timestep or step_dev' in texts[t]
    assert 'sr3_unet_forward_full: t_map goes with step_dev' in texts['FORWARD_FULL']
    for t in ('STEP', 'STEP_EX', 'STEP_HIST'):
        assert 'SR3 variant needs level_table' in texts[t]
    assert sum('reverse_step' in m for m in texts['STEP_HIST']) >= 6       # check_step_history's own refusals
    for word in ('store_wt -1', 'store_wt 8', 'gemm_epi 3', 'var_channels 1', 'attn_heads 0: needs a value >= 1', 'attn_head_dim -1: needs a value >= 0',
                 'mutually exclusive', 'needs a divisor with a head width', 'needs a multiple of 4 that divides them', 'unknown option nonsense', 'bad param index'):
        assert any(word in m for m in texts['OPTION']), word
    assert all('must be positive multiples of' in m or m == 'null plan' for m in texts['GEOMETRY'])
    for word in ('null plan', 'derived buffer too small', 'not 16-byte aligned', 'null argument', 'no derived buffer bound'):
        assert any(word in m for m in texts['DERIVED']), word


def test_the_order_of_checks_is_the_recorded_one(recorded):
    """the fixture itself says which of two faults each entry reports"""
    def text(table, net, **kw):
        for i, (_, n, row) in enumerate(TABLES[table]):
            if n == net and {k: getattr(v, 'value', v) for k, v in row.items()} == {k: getattr(v, 'value', v) for k, v in kw.items()}:
                return recorded['%s[%d]' % (table, i)][1]
        raise KeyError((table, net, kw))
    for t in ('FORWARD', 'FORWARD_FULL'):
        assert text(t, 'sr3_tiny', x=None, batch=0) == 'null argument'                                  # null arguments before the build
        assert text(t, 'sr3_tiny', batch=0, ws_short=1) == 'batch must be > 0'                          # the build before the workspace size
        assert 'out of range' in text(t, 'ddpm_tiny', cond=_p(2), cc=-1, ws=_p(WS, 4))
        assert 'too small' in text(t, 'sr3_tiny', ws_short=1, ws=_p(WS, 4))                             # size before alignment
        assert 'too small' in text(t, 'sr3_tiny', ws_short=1, level=None, tstep=None)
        assert 'misaligned' in text(t, 'ddpm_tiny', x=_p(1, 4), level=None, tstep=None)                 # alignment before what the variant needs
    assert 't_map' in text('FORWARD_FULL', 'sr3_tiny', t_map=_p(20), x=None)                            # the entry's own check first
    for t in ('STEP', 'STEP_EX', 'STEP_HIST'):
        assert text(t, 'sr3_tiny', ta=None, batch=0) == 'null argument'
        assert 'too small' in text(t, 'sr3_tiny', ws_short=1, z=_p(10, 4))
        assert 'misaligned' in text(t, 'sr3_tiny', z=_p(10, 4), level_table=None)
    assert text('STEP_HIST', 'sr3_tiny', level_table=None, c3=_p(21)) == 'SR3 variant needs level_table'      # ... before the history pair
    assert 'misaligned' in text('STEP_HIST', 'ddpm_tiny', z=_p(10, 4), hist=_p(22))
    assert text('PROFILE', 'sr3_tiny', op_ms=None, batch=0) == 'null argument'
    assert text('PROFILE', 'sr3_tiny', batch=0, ws_short=1) == 'batch must be > 0'


@pytest.mark.parametrize('table,case', CASES, ids=['%s-%d' % c for c in CASES])
def test_refusal_is_the_recorded_one(recorded, table, case):
    from helpers import experiments_built
    from sr3_hip import lib as L
    got = _call(L.load(), table, case)
    if table == 'OPTION' and TABLES[table][case][2][1] == 'split_bf16' and experiments_built():
        assert got[0] == 0      # (an experiments build takes the option; the default build's refusal is the recorded one)
        return
    assert got[0] < 0, (table, case, got)      # (a refusal: nothing was launched)
    assert got == recorded['%s[%d]' % (table, case)], (table, case)


# ---- the derived-buffer preflight ------------------------------------------------------------------------------------------------------

NOT_BOUND = "the plan's derived (Winograd) weights are not bound: call sr3_plan_bind_derived + sr3_plan_prepare_derived"
STALE = "the plan's derived (Winograd) weights are stale or were prepared from another arena: call sr3_plan_prepare_derived"
WSPLIT = "the plan's derived (pre-split 1x1 / stride-2) weights are not bound or stale: call sr3_plan_bind_derived + sr3_plan_prepare_derived"
RUN_ENTRIES = ('sr3_unet_forward', 'sr3_unet_forward_full', 'sr3_reverse_step', 'sr3_reverse_step_ex', 'sr3_reverse_step_hist')


W64 = ('sr3', 6, 3, 64, 32, [1, 2], [8], 1, 16)      # Winograd convs and plain-GEMM convs (pre-split weights) on one small list
WINO_TILES, GEMM_TILES = (11, 12, 13, 23, 25, 26), (18, 19, 20, 21, 22)


def _derived_kinds(plan):
    """'w' / 'g' per conv of the launch list that reads the derived buffer: Winograd filters / pre-split GEMM weights, in list order"""
    return ['w' if o['tile_cfg'] in WINO_TILES else 'g' for o in plan.op_list(B) if o['kind'] == 50 and o['tile_cfg'] in WINO_TILES + GEMM_TILES]


def _refused(plan, entry):
    """[return code, text] of `entry` on `plan` with made-up aligned pointers and a workspace of the queried size"""
    _plans['preflight'] = (plan, plan.workspace_bytes(B))      # (_run_args' defaults suit every conditional SR3 network)
    try:
        assert plan.lib.sr3_plan_param_info(None, 0, None) == BADARG
        rc = getattr(plan.lib, entry)(*_run_args(entry, 'preflight'))
        return [int(rc), plan.lib.sr3_last_error().decode()]
    finally:
        del _plans['preflight']


@pytest.mark.parametrize('entry', RUN_ENTRIES)
def test_forward_without_derived_filters_is_refused_before_any_launch(entry):
    """A forward whose launch list holds a Winograd conv, on a plan with no derived buffer bound (then: bound, never prepared), with made-up
    aligned pointers and a sufficient size: SR3_E_BADARG and the text, with no HIP call -- this machine has no device, and a made-up
    address never reaches a kernel.  While the two checks sat inside the launch loop's conv case, the same call on a machine without a
    GPU failed with a HIP error from the first launch (the embedding kernel, the input conv and the statistics passes in front of the
    first Winograd conv were enqueued before the refusal; under stream capture that left a half-built graph): that difference is the
    evidence that the refusal now precedes every launch."""
    from sr3_hip import engine as E
    plan = E.Plan(*W64)
    assert _derived_kinds(plan)[0] == 'w', 'the first conv that reads the derived buffer is not a Winograd conv'
    assert _refused(plan, entry) == [BADARG, NOT_BOUND]
    assert plan.lib.sr3_plan_bind_derived(plan.handle, _p(30), int(plan.lib.sr3_plan_derived_bytes(plan.handle))) == 0
    assert _refused(plan, entry) == [BADARG, STALE]


def test_preflight_asks_what_each_op_asked():
    """winograd = 0 leaves the pre-split GEMM weights as the only derived operand: their text (one for unbound and stale), not the
    Winograd one; a plan that reads no derived operand at all is not refused for the missing buffer."""
    from sr3_hip import engine as E
    plan = E.Plan(*W64)
    plan.set_option('winograd', 0)
    assert set(_derived_kinds(plan)) == {'g'}, 'no plain-GEMM conv on the list'
    assert _refused(plan, 'sr3_unet_forward') == [BADARG, WSPLIT]
    assert plan.lib.sr3_plan_bind_derived(plan.handle, _p(30), int(plan.lib.sr3_plan_derived_bytes(plan.handle))) == 0
    assert _refused(plan, 'sr3_reverse_step') == [BADARG, WSPLIT]


# ---- options on a plan that has already built its lists --------------------------------------------------------------------------------

SR3_16_128 = ('sr3', 6, 3, 64, 32, [1, 2, 4, 8, 8], [16], 2, 128)
# every key sr3_plan_set_option takes, with a value that is not its default
OPTION_VALUES = [
    ('fuse_stats', 0), ('tile_cfg', 5), ('ksplit', 2), ('keep_all', 1), ('fuse_res', 0), ('split_bf16', 1), ('winograd', 0), ('wino_split', 0),
    ('wino_split8', 0), ('wgrad_split', 0), ('attn_split', 0), ('store_wt', 0), ('gemm_epi', 0), ('attn_long', 1), ('gemm_split', 0), ('gemm_wpre', 1),
    ('gemm2', 0), ('gemm_s2', 0), ('fork_side', 1), ('gemm_n64', 0), ('fold_fuse', 0), ('gemm_tile', 2), ('wino2', 0), ('wino_ragged', 0),
    ('wino_up', 0), ('train_geom', 1), ('loss_l2', 1), ('var_channels', 3), ('attn_heads', 2), ('attn_head_dim', 32),
]
SEQ_BATCH = 4


def test_the_option_list_names_every_key_the_library_takes():
    """counted by probing: every lower-case word of the public header, asked of a fresh plan"""
    from sr3_hip import lib as L
    lib = L.load()
    with open(HEADER) as f:
        words = sorted(set(re.findall(r'[a-z][a-z0-9_]*', f.read())))
    taken = []
    for w in words:
        plan = _fresh('sr3_tiny')
        rc = lib.sr3_plan_set_option(plan.handle, w.encode(), 0)
        if rc >= 0 or not lib.sr3_last_error().decode().startswith('unknown option'):
            taken.append(w)
    assert len(OPTION_VALUES) == len(taken) and sorted(k for k, _ in OPTION_VALUES) == taken, sorted(set(taken) ^ {k for k, _ in OPTION_VALUES})


def _state(plan):
    lib, h = plan.lib, plan.handle
    n = int(lib.sr3_plan_num_ops(h, SEQ_BATCH))
    ops = plan.op_list(SEQ_BATCH) if n >= 0 else ('refused', lib.sr3_last_error().decode())
    train = int(lib.sr3_train_workspace_bytes(h, SEQ_BATCH, 3))
    return dict(ops=ops, ws=int(lib.sr3_workspace_bytes(h, SEQ_BATCH)), derived=int(lib.sr3_plan_derived_bytes(h)), train=train,
                train_refused=lib.sr3_last_error().decode() if train == 0 else '')


_untouched = {}


def _net_for(key):
    """the plan of sr3_16_128; var_channels needs a variance head: the same network with out_channel 6"""
    return SR3_16_128[:2] + (6,) + SR3_16_128[3:] if key == 'var_channels' else SR3_16_128


@pytest.mark.parametrize('key,value', OPTION_VALUES, ids=['%s=%d' % kv for kv in OPTION_VALUES])
def test_option_set_after_the_lists_were_built(key, value):
    """Set on a plan that has built its forward and its training plan, an option leaves what a fresh plan created with it builds; set
    back to its default, what the untouched plan built.  (The plan fingerprint only ever sets options on fresh plans.)"""
    from helpers import experiments_built
    from sr3_hip import engine as E, lib as L
    args = _net_for(key)
    if args[2] not in _untouched:
        _untouched[args[2]] = _state(E.Plan(*args))
    untouched = _untouched[args[2]]
    plan = E.Plan(*args)
    assert _state(plan) == untouched
    if key == 'split_bf16' and not experiments_built():
        with pytest.raises(L.Sr3Error, match='SR3_EXPERIMENTS'):
            plan.set_option(key, value)
        assert _state(plan) == untouched
        return
    default = plan.set_option(key, value)
    assert default != value, 'the value under test is the default'
    fresh = E.Plan(*args)
    fresh.set_option(key, value)
    assert _state(plan) == _state(fresh), key
    assert plan.set_option(key, default) == value
    assert _state(plan) == untouched, key


if __name__ == '__main__':
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, 'image-super-resolution-via-iterative-refinement_amd'), HERE]
    from sr3_hip import lib as L
    lib = L.load()
    out = {'%s[%d]' % c: _call(lib, *c) for c in CASES}
    bad = [k for k, v in out.items() if v[0] >= 0]
    assert not bad, 'not refused (a launch was attempted): %s' % bad
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d refusals from %s' % (len(out), L.LIB_PATH))
