"""`EngineDiffusion._step_rule`, host side (no GPU): what the one step method runs on -- the schedule's own buffers for the ancestral
sampler (the very tensors, so the ancestral loop's engine call and captured graph are what they were), the `_sampler_*` tables under a
sampler, the timestep map for the DDPM variant only, c3 for the multistep solver only, noise only where eta > 0.  T = 8."""
import pytest
import torch

from helpers import SCHEDS, opt_for

SCHED = SCHEDS['sr3_tiny']


@pytest.fixture(scope='module')
def nets():
    import model as Model
    out = {}
    for name in ('sr3_tiny', 'ddpm_tiny'):
        netG = Model.create_model(opt_for(name, gpu=False)).netG
        netG.set_new_noise_schedule(dict(SCHED), torch.device('cpu'))
        assert netG.num_timesteps == 8
        out[netG.variant] = netG
    assert set(out) == {'sr3', 'ddpm'}
    return out


def _sampler_five(netG):
    return [getattr(netG, '_sampler_' + k) for k in ('a', 'b', 'c1', 'c2', 'sigma')]


@pytest.mark.parametrize('variant', ['sr3', 'ddpm'])
def test_no_sampler_is_the_schedules_own_buffers(nets, variant):
    netG = nets[variant]
    netG.set_sampler(None)
    tables, level, t_map, c3, noisy = netG._step_rule()
    own = (netG.sqrt_recip_alphas_cumprod, netG.sqrt_recipm1_alphas_cumprod, netG.posterior_mean_coef1, netG.posterior_mean_coef2,
           netG._sigma)
    assert len(tables) == 5
    assert [t.data_ptr() for t in tables] == [t.data_ptr() for t in own] and all(t.shape == (8,) for t in tables)
    assert level.data_ptr() == netG._level_table.data_ptr() and level.shape == (9,)
    assert t_map is None and c3 is None and noisy is True


def test_ddim_on_sr3_gives_the_sampler_tables_and_noise_follows_eta(nets):
    netG = nets['sr3']
    for eta, want in ((0.0, False), (0.5, True)):
        netG.set_sampler(4, eta)
        tables, level, t_map, c3, noisy = netG._step_rule()
        assert len(tables) == 5 and all(a is b for a, b in zip(tables, _sampler_five(netG))) and all(t.shape == (4,) for t in tables)
        assert level is netG._sampler_level and level.shape == (5,)
        assert t_map is None and c3 is None and noisy is want
    netG.set_sampler(None)


def test_ddpm_variant_gets_the_timestep_map(nets):
    netG = nets['ddpm']
    netG.set_sampler(4, 0.0)
    tables, level, t_map, c3, noisy = netG._step_rule()
    assert t_map is netG._sampler_tau and t_map.dtype == torch.int32 and t_map.tolist() == [0, 2, 5, 7]
    assert all(a is b for a, b in zip(tables, _sampler_five(netG))) and c3 is None and noisy is False
    netG.set_sampler(None)


def test_multistep_solver_gets_c3(nets):
    netG = nets['sr3']
    netG.set_sampler(4, kind='dpmpp_2m')
    tables, level, t_map, c3, noisy = netG._step_rule()
    assert c3 is not None and c3 is netG._sampler_c3 and c3.shape == (4,)
    assert all(a is b for a, b in zip(tables, _sampler_five(netG))) and level is netG._sampler_level
    assert t_map is None and noisy is False
    netG.set_sampler(None)
