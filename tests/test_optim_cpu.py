"""Gradient accumulation and global-norm clipping, the parts that need no GPU: the micro-batch schedule, the validation of the two
config keys (train.optimizer.accumulate / clip_grad_norm), and the four new entry points in the header, the library and lib.py."""
import os
import re

import pytest

from helpers import ROOT, opt_for

NEW_ENTRIES = ('sr3_grad_norm_scratch_bytes', 'sr3_grad_norm', 'sr3_grad_accumulate', 'sr3_adam_ema_step_scaled')


@pytest.mark.parametrize('K', [1, 2, 3])
def test_schedule_over_seven_micro_batches(K):
    from sr3_hip.optim import accumulate_schedule
    got = [accumulate_schedule(i, K) for i in range(7)]
    assert got == [(i % K == 0, i % K == K - 1) for i in range(7)]
    assert sum(1 for _, last in got if last) == 7 // K
    # every sum that is closed was opened exactly once before, and nothing is open twice
    open_ = False
    for first, last in got:
        assert first != open_
        open_ = not last


def build(**optimizer_keys):
    import model as Model
    opt = opt_for('sr3_tiny', phase='train', gpu=False)
    opt['train']['optimizer'].update(optimizer_keys)
    return Model.create_model(opt)


@pytest.mark.parametrize('key,value', [('accumulate', 0), ('accumulate', -1), ('accumulate', 2.5), ('accumulate', True),
                                       ('clip_grad_norm', 0), ('clip_grad_norm', -1), ('clip_grad_norm', float('nan'))])
def test_bad_config_values_raise_naming_the_key(key, value):
    with pytest.raises(ValueError) as e:
        build(**{key: value})
    assert 'train.optimizer.' + key in str(e.value)


def test_absent_keys_leave_both_off():
    m = build()
    assert m.optG.accumulate == 1 and m.optG.clip_grad_norm is None
    assert m.optG.grad_acc is None and m.optG.norm4 is None and m.optG.last_grad_norm() is None
    assert m.netG.denoise_fn.accumulate == 1
    m = build(accumulate=None, clip_grad_norm=None)              # a JSON null is an absent key
    assert m.optG.accumulate == 1 and m.optG.clip_grad_norm is None


def test_given_keys_are_taken():
    m = build(accumulate=4, clip_grad_norm=1)
    assert m.optG.accumulate == 4 and m.optG.clip_grad_norm == 1.0 and isinstance(m.optG.clip_grad_norm, float)
    assert m.netG.denoise_fn.accumulate == 4
    assert m.optG.grad_acc is None and m.optG.norm4 is None      # nothing is allocated before the first step
    # neither key, nor the position inside an accumulation, is part of the optimizer's checkpoint
    sd = m.optG.state_dict()
    assert set(sd) == {'state', 'param_groups'} and 'accumulate' not in sd['param_groups'][0]
    m.optG.micro_count = 3
    m.optG.load_state_dict(sd)
    assert m.optG.micro_count == 0


def test_new_entries_are_declared_exported_and_bound():
    """The mechanism of tests/test_abi_cpu.py, for the four new names."""
    from sr3_hip import lib as L
    src = open(os.path.join(ROOT, 'include', 'sr3_mi355x.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(sr3_[a-z0-9_]+)\s*\(', src))
    lib = L.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert len(L.SIGNATURES['sr3_adam_ema_step_scaled'][1]) == len(L.SIGNATURES['sr3_adam_ema_step'][1]) + 1
    assert lib.sr3_version() == 1                                # additive: the ABI version does not move
    # the scratch query is host-only: at most one double per block of the fixed grid, and one block for a tiny array
    assert lib.sr3_grad_norm_scratch_bytes(4) == 8
    big = lib.sr3_grad_norm_scratch_bytes(1 << 30)
    assert big == lib.sr3_grad_norm_scratch_bytes(1 << 28) and big % (256 * 8) == 0
