"""EMA of the weights and learning-rate warm-up, the parts that need no GPU (gpu=False models: construction and checkpoint I/O
work there): the opt-in switch (train.ema_scheduler.enabled), the `*_ema.pth` file, the three resume cases and the warm-up
schedule."""
import logging
import os

import pytest
import torch

from helpers import opt_for

REF_EMA = {'step_start_ema': 5000, 'update_ema_every': 1, 'ema_decay': 0.9999}      # what every reference config carries


def make(tmp_path, phase='train', ema=None, resume=None, seed=3):
    import model as Model
    opt = opt_for('sr3_tiny', phase=phase, gpu=False)
    opt['path']['checkpoint'] = str(tmp_path)
    opt['path']['resume_state'] = resume
    if ema is not None:
        opt['train']['ema_scheduler'] = dict(ema)
    torch.manual_seed(seed)
    return Model.create_model(opt)


def unet_part(sd):
    return {k: v for k, v in sd.items() if k.startswith('denoise_fn.')}


@pytest.mark.parametrize('ema', [REF_EMA, dict(REF_EMA, enabled=False)], ids=['reference_block', 'enabled_false'])
def test_ema_off_changes_nothing(tmp_path, ema):
    base = make(tmp_path / 'none')
    m = make(tmp_path, ema=ema)
    un = m.netG.denoise_fn
    assert un.ema_arena is None and m.optG.ema is None and m.optG.warmup_steps == 0
    m.save_network(epoch=1, iter_step=5)
    assert sorted(os.listdir(tmp_path)) == ['I5_E1_gen.pth', 'I5_E1_opt.pth']
    assert list(m.netG.state_dict().keys()) == list(base.netG.state_dict().keys())
    assert [k for k, _ in m.netG.named_parameters()] == [k for k, _ in base.netG.named_parameters()]
    assert m.optG.state_dict().keys() == base.optG.state_dict().keys()
    from sr3_hip import lib as L
    with pytest.raises(L.Sr3Error):
        un.ema_state_dict()
    with pytest.raises(L.Sr3Error):
        with un.use_weights('ema'):
            pass


def test_ema_on_fresh_model_and_file(tmp_path):
    m = make(tmp_path, ema=dict(REF_EMA, enabled=True))
    off = make(tmp_path / 'off')
    un = m.netG.denoise_fn
    sd = m.netG.state_dict()
    # not a parameter, not a buffer: the state dict, the parameter list and the printed count are those of a model without EMA
    assert list(sd.keys()) == list(off.netG.state_dict().keys())
    assert [k for k, _ in m.netG.named_parameters()] == [k for k, _ in off.netG.named_parameters()]
    assert m.get_network_description(m.netG)[1] == off.get_network_description(off.netG)[1]
    assert all(b is not un.ema_arena for b in m.netG.buffers())
    # the EMA starts as the weights the model starts from
    ema = un.ema_state_dict('denoise_fn.')
    assert ema.keys() == unet_part(sd).keys()
    assert all(torch.equal(ema[k], sd[k]) for k in ema)
    assert un.ema_arena.data_ptr() != un.arena.data_ptr()
    m.save_network(epoch=2, iter_step=7)
    assert sorted(os.listdir(tmp_path)) == ['I7_E2_ema.pth', 'I7_E2_gen.pth', 'I7_E2_opt.pth']
    gen = torch.load(tmp_path / 'I7_E2_gen.pth', map_location='cpu')
    ema = torch.load(tmp_path / 'I7_E2_ema.pth', map_location='cpu')
    assert list(ema.keys()) == list(gen.keys())
    assert all(ema[k].shape == gen[k].shape and ema[k].dtype == gen[k].dtype for k in gen)
    assert all(torch.equal(ema[k], gen[k]) for k in gen)
    # the optimizer file keeps torch.optim.Adam's format: no EMA or warm-up entry
    ck = torch.load(tmp_path / 'I7_E2_opt.pth', map_location='cpu')
    assert sorted(ck.keys()) == ['epoch', 'iter', 'optimizer', 'scheduler']
    assert sorted(ck['optimizer'].keys()) == ['param_groups', 'state']


def perturbed_checkpoint(tmp_path):
    """A train-phase model with EMA whose EMA arena differs from its weights, saved as I7_E2."""
    m = make(tmp_path, ema=dict(REF_EMA, enabled=True))
    un = m.netG.denoise_fn
    ptr = un.ema_arena.data_ptr()
    un.ema_arena.add_(torch.randn(un.ema_arena.shape, generator=torch.Generator().manual_seed(11)) * 0.01)
    assert un.ema_arena.data_ptr() == ptr
    m.save_network(epoch=2, iter_step=7)
    return m, str(tmp_path / 'I7_E2')


def test_resume_train_phase_restores_ema(tmp_path):
    m, stem = perturbed_checkpoint(tmp_path)
    m2 = make(tmp_path, ema=dict(REF_EMA, enabled=True), resume=stem, seed=99)
    a, b = m.netG.state_dict(), m2.netG.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)                      # live weights: *_gen.pth
    ea, eb = m.netG.denoise_fn.ema_state_dict('denoise_fn.'), m2.netG.denoise_fn.ema_state_dict('denoise_fn.')
    assert ea.keys() == eb.keys() == unet_part(a).keys()
    assert all(torch.equal(ea[k], eb[k]) for k in ea)                   # EMA weights: *_ema.pth (every entry; the arena's alignment
    assert all(not torch.equal(eb[k], b[k]) for k in eb)               # padding between entries is in no file)
    assert m2.begin_step == 7 and m2.begin_epoch == 2


def test_resume_val_phase_loads_ema_weights(tmp_path):
    m, stem = perturbed_checkpoint(tmp_path)
    v = make(tmp_path, phase='val', ema=dict(REF_EMA, enabled=True), resume=stem, seed=99)
    assert v.netG.denoise_fn.ema_arena is None                          # the EMA weights are the model's weights: one arena
    ema = m.netG.denoise_fn.ema_state_dict('denoise_fn.')
    got = v.netG.state_dict()
    assert all(torch.equal(got[k], ema[k]) for k in ema)
    # without `enabled` the same checkpoint gives the raw weights, as before
    raw = make(tmp_path, phase='val', ema=REF_EMA, resume=stem, seed=99).netG.state_dict()
    live = m.netG.state_dict()
    assert all(torch.equal(raw[k], live[k]) for k in live)
    os.remove(stem + '_ema.pth')
    with pytest.raises(FileNotFoundError) as e:
        make(tmp_path, phase='val', ema=dict(REF_EMA, enabled=True), resume=stem)
    assert 'I7_E2_ema.pth' in str(e.value)


def test_resume_train_phase_without_ema_file_warns(tmp_path, caplog):
    m, stem = perturbed_checkpoint(tmp_path)
    os.remove(stem + '_ema.pth')
    with caplog.at_level(logging.WARNING, logger='base'):
        m2 = make(tmp_path, ema=dict(REF_EMA, enabled=True), resume=stem, seed=99)
    assert any(r.levelno == logging.WARNING and 'I7_E2_ema.pth' in r.getMessage() for r in caplog.records)
    un = m2.netG.denoise_fn
    assert torch.equal(un.ema_arena, un.arena.data) and un.ema_arena.data_ptr() != un.arena.data_ptr()
    assert torch.equal(un.arena.data, m.netG.denoise_fn.arena.data)


def test_warmup_schedule_and_ema_rule():
    from sr3_hip.optim import ema_mode, warmup_lr
    lr = 1e-4
    assert [warmup_lr(lr, s, 4) for s in range(1, 6)] == [lr / 4, lr / 2, 3 * lr / 4, lr, lr]
    assert [warmup_lr(lr, s, 0) for s in range(1, 6)] == [lr] * 5
    # the EMA rule on the 1-based step count: untouched off the update steps, a copy before step_start_ema, the lerp from there on
    assert [ema_mode(s, 3, 1) for s in range(1, 6)] == [1, 1, 2, 2, 2]
    assert [ema_mode(s, 4, 2) for s in range(1, 8)] == [0, 1, 0, 2, 0, 2, 0]


def test_config_keys_reach_the_optimizer(tmp_path):
    import model as Model
    opt = opt_for('sr3_tiny', phase='train', gpu=False)
    opt['path']['checkpoint'] = str(tmp_path)
    opt['train']['optimizer']['warmup_steps'] = 4
    opt['train']['ema_scheduler'] = dict(REF_EMA, enabled=True)
    m = Model.create_model(opt)
    assert m.optG.warmup_steps == 4
    assert m.optG.ema == REF_EMA
    assert m.optG.state_dict()['param_groups'][0]['lr'] == 1e-4       # the base learning rate, whatever the step
    lib_sig = __import__('sr3_hip.lib', fromlist=['SIGNATURES']).SIGNATURES
    assert len(lib_sig['sr3_adam_ema_step'][1]) == 14
