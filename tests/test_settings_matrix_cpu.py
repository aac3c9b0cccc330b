"""What the settings of EngineDiffusion accept and refuse together, as a matrix (CPU only: no call reaches a launch).

For each of seven tiny models every setting is switched off, then every ordered sequence of 1, 2 and 3 distinct setter calls out of
eleven is applied; what the LAST call of the sequence gave -- 'ok', or the exception's type name and whole message -- is the entry (the
calls before it are a shorter sequence of the table, from the same start).  The 1- and 2-call sequences are then repeated with a
p_sample_loop_tiled(..., tile=16, overlap=4) call behind them: on a CPU model it always fails, and the entry says which refusal wins
before "needs the model on a GPU" -- the loop's own check of the settings against the tiling it was handed.

tests/settings_matrix.json holds the table as it was recorded from the code before the setters shared one compatibility check
(`EngineDiffusion._check_settings`): whatever checks the settings has to refuse the same calls with the same type and text.  An entry
may list more than one outcome -- a call that breaks two rules at once, where either rule's message is right; the test takes any.

Record again (only from code whose refusals are the wanted ones):  python tests/test_settings_matrix_cpu.py --record
"""
import copy
import itertools
import json
import os
import sys

import torch

from helpers import opt_for

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'settings_matrix.json')

# name -> (config of helpers.opt_for, unet keys, diffusion keys)
MODELS = {
    'sr3_tiny': ('sr3_tiny', {}, {}),
    'sr3_tiny_in9': ('sr3_tiny', dict(in_channel=9), {}),
    'sr3_tiny_in7': ('sr3_tiny', dict(in_channel=7), {}),
    'sr3_tiny_out6_lv': ('sr3_tiny', dict(out_channel=6), dict(learned_variance={'lambda': 0.001})),
    'sr3_tiny_in9_out6_lv': ('sr3_tiny', dict(in_channel=9, out_channel=6), dict(learned_variance={'lambda': 0.001})),
    'ddpm_tiny': ('ddpm_tiny', {}, {}),
    'sr3_uncond_in6': ('sr3_uncond', dict(in_channel=6), {}),
}

CALLS = (
    ('ddim', lambda n: n.set_sampler(4, 0.0, kind='ddim')),
    ('dpmpp_2m', lambda n: n.set_sampler(4, 0.0, kind='dpmpp_2m')),
    ('ancestral', lambda n: n.set_sampler(4, kind='ancestral')),
    ('tiling', lambda n: n.set_tiling(16, 4)),
    ('consistency', lambda n: n.set_consistency(4)),
    ('guidance', lambda n: n.set_guidance(1.5)),
    ('backprojection', lambda n: n.set_backprojection(4)),
    ('self_condition', lambda n: n.set_self_condition(0.5)),
    ('cond_augment', lambda n: n.set_cond_augment(0.5, 0.1, True)),
    ('cond_augment_blind', lambda n: n.set_cond_augment(0.5, 0.1, False)),
    ('learned_variance', lambda n: n.set_learned_variance(0.001)),
)
LOOP = 'loop_tiled'


def build(name):
    from model import networks
    base, unet, diffusion = MODELS[name]
    opt = opt_for(base, phase='val', gpu=False)
    opt['model']['unet'].update(unet)
    opt['model']['diffusion'].update(diffusion)
    netG = networks.define_G(copy.deepcopy(opt))
    netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], torch.device('cpu'))
    netG.show_progress = False
    return netG


def reset(netG):
    """every setting off, by the attributes: no setter's check stands in the way"""
    netG.learned_variance = None
    netG.set_sampler(None)
    for k in ('tiling', 'consistency', 'guidance', 'backprojection', 'self_condition', 'cond_augment'):
        setattr(netG, k, None)
    netG._loop_cache = {}


def loop_tiled(netG):
    shape = (2, 3, 32, 32)
    netG.p_sample_loop_tiled(torch.zeros(shape) if netG.conditional else shape, tile=16, overlap=4)


def outcome(fn, netG):
    try:
        fn(netG)
    except Exception as e:      # noqa: BLE001  (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return 'ok'


def run(netG):
    """{'call|call|...': the last call's outcome} over every sequence of the module's docstring"""
    calls = dict(CALLS)
    out = {}
    for n in (1, 2, 3):
        for seq in itertools.permutations(calls, n):
            for tail in ((), (LOOP,)) if n < 3 else ((),):
                reset(netG)
                for name in seq[:-1] if not tail else seq:
                    outcome(calls[name], netG)
                out['|'.join(seq + tail)] = outcome(loop_tiled if tail else calls[seq[-1]], netG)
    return out


DIGITS = '0123456789abcdefghijklmnopqrstuvwxyz'
WIDTH = 112      # sequences per line of the table


def sequences():
    """the keys of `run`, in its order"""
    calls = [c for c, _ in CALLS]
    return ['|'.join(seq + tail) for n in (1, 2, 3) for seq in itertools.permutations(calls, n)
            for tail in (((), (LOOP,)) if n < 3 else ((),))]


def record():
    """The table: {'outcomes': every distinct outcome once, 'models': {model: lines of one digit per sequence, in `sequences()`'s order
    -- the outcome's index, base 36}, 'either': {model: {sequence: digits}} for the sequences where more than one outcome is right}."""
    outcomes, models = ['ok'], {}
    for name in MODELS:
        got = run(build(name))
        assert list(got) == sequences()
        for o in got.values():
            if o not in outcomes:
                outcomes.append(o)
        row = ''.join(DIGITS[outcomes.index(o)] for o in got.values())
        models[name] = [row[i:i + WIDTH] for i in range(0, len(row), WIDTH)]
    assert len(outcomes) <= len(DIGITS)
    return dict(outcomes=outcomes, models=models, either={})


def _table():
    """-> {model: {sequence: [the outcomes that are right]}}"""
    with open(FIXTURE) as f:
        tab = json.load(f)
    out = {}
    for name, lines in tab['models'].items():
        row = ''.join(lines)
        assert len(row) == len(sequences()), name
        out[name] = {k: [tab['outcomes'][DIGITS.index(d)] for d in row[i] + tab['either'].get(name, {}).get(k, '')]
                     for i, k in enumerate(sequences())}
    return out


def test_every_model_and_sequence_is_in_the_table():
    tab = _table()
    n_seq = 11 + 11 * 10 + 11 * 10 * 9
    assert sorted(tab) == sorted(MODELS)
    for name, rows in tab.items():
        assert len(rows) == n_seq + 11 + 11 * 10, name
        assert sum(1 for k in rows if not k.endswith(LOOP)) == n_seq == 1111
        assert all(o != 'ok' for k, v in rows.items() if k.endswith(LOOP) for o in v), name      # the loop never starts


def test_settings_matrix_matches_the_recorded_table():
    tab = _table()
    bad = []
    for name in MODELS:
        got = run(build(name))
        want = tab[name]
        assert sorted(got) == sorted(want), name
        bad += [(name, k, o, want[k]) for k, o in got.items() if o not in want[k]]
    assert not bad, '%d of the sequences differ from the table; the first: %r' % (len(bad), bad[:3])


if __name__ == '__main__':
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd'), os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    if '--record' not in sys.argv[1:]:
        sys.exit('usage: python tests/test_settings_matrix_cpu.py --record')
    with open(FIXTURE, 'w') as f:
        json.dump(record(), f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded', FIXTURE)
