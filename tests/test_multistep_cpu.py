"""The second-order multistep sampler, host side (no GPU): `sr3_hip.diffusion.sampler_walk` and the `kind` / `walk` keywords of
`sampler_tables` -- that the defaults are the DDIM tables they were, the properties of the log-SNR walk, the DPM-Solver++(2M) tables
against DDIM's where the two must agree, the accuracy of the pair (2M tail + log-SNR walk) on a toy problem with an exact solution,
and the config surface.  Everything is float64 numpy."""
import numpy as np
import pytest
import torch

from helpers import SCHEDS, opt_for


def _ac(T, lo, hi):
    return np.cumprod(1.0 - np.linspace(lo, hi, T, dtype=np.float64))


# the two schedules of DESIGN.md 3.1n's table and the sr3_tiny fixture's own (T = 8: every small-S corner)
LINEAR = [(2000, 1e-6, 1e-2), (1000, 1e-4, 2e-2), (8, 1e-6, 1e-2)]
TABLE = LINEAR[:2]


def _lam(ac):
    return 0.5 * np.log(ac / (1.0 - ac))


def _ddim_tables_before(ac, S, eta):
    """The body of sampler_tables as it stood before the `kind` / `walk` keywords, restated: what the defaults must still return."""
    T = ac.shape[0]
    tau = np.round(np.linspace(0, T - 1, S)).astype(np.int64) if S > 1 else np.array([T - 1], dtype=np.int64)
    ab = ac[tau]
    ap = np.append(1.0, ab[:-1])
    sigma = eta * np.sqrt((1.0 - ap) / (1.0 - ab)) * np.sqrt(1.0 - ab / ap)
    d = np.sqrt(np.maximum(1.0 - ap - sigma ** 2, 0.0))
    return dict(tau=tau, a=np.sqrt(1.0 / ab), b=np.sqrt(1.0 / ab - 1), c1=np.sqrt(ap) - d * np.sqrt(ab) / np.sqrt(1.0 - ab),
                c2=d / np.sqrt(1.0 - ab), sigma=sigma, level=np.append(1.0, np.sqrt(ab)))


@pytest.mark.parametrize('eta', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('T,lo,hi', TABLE)
def test_defaults_are_the_ddim_tables_bit_for_bit(T, lo, hi, eta):
    from sr3_hip.diffusion import sampler_tables, sampler_walk
    ac = _ac(T, lo, hi)
    for S in (1, 2, 7, T):
        want = _ddim_tables_before(ac, S, eta)
        for got in (sampler_tables(ac, S, eta), sampler_tables(ac, S, eta, kind='ddim', walk='time')):
            assert set(got) == set(want) | {'c3'}
            for k, v in want.items():
                assert got[k].dtype == v.dtype and np.array_equal(got[k], v), (S, k)
            assert got['c3'].shape == (S,) and got['c3'].dtype == np.float64 and not got['c3'].any()
        tau = sampler_walk(ac, S, 'time')
        assert tau.dtype == np.int64 and np.array_equal(tau, want['tau'])
    assert np.array_equal(sampler_walk(ac, 5), sampler_walk(ac, 5, 'time'))


@pytest.mark.parametrize('T,lo,hi', LINEAR)
def test_walks(T, lo, hi):
    """Both walks: int64 [S], strictly increasing, ends pinned, identity at S = T, S = 1 -> [T - 1], S > T refused.  The log-SNR walk is
    uniform in lambda as far as a discrete schedule lets it be: where tau[i] is the timestep nearest its target (i.e. away from the
    ends the two passes force), lambda(tau[i]) misses the target by at most half the larger of the two lambda gaps next to tau[i]
    (nearest-neighbour rounding), so the gap between two such neighbours differs from the targets' uniform spacing by at most the sum
    of the two half gaps."""
    from sr3_hip.diffusion import sampler_walk
    ac = _ac(T, lo, hi)
    lam = _lam(ac)
    assert np.all(np.diff(lam) < 0)
    local = np.abs(np.diff(lam))
    half = 0.5 * np.maximum(np.append(local, 0.0), np.append(0.0, local))      # half the larger gap next to each timestep
    for walk in ('time', 'logsnr'):
        for S in sorted({1, 2, 3, 10, 40, T} & set(range(1, T + 1))):
            tau = sampler_walk(ac, S, walk)
            assert tau.dtype == np.int64 and tau.shape == (S,) and tau[-1] == T - 1, (walk, S)
            if S > 1:
                assert tau[0] == 0 and np.all(np.diff(tau) > 0), (walk, S)
            if S == T:
                assert np.array_equal(tau, np.arange(T))
            if walk == 'logsnr' and S > 2:
                target = np.linspace(lam[0], lam[-1], S)
                nearest = np.array([int(np.argmin(np.abs(lam - v))) for v in target])
                free = tau == nearest
                assert np.all(np.abs(lam[tau[free]] - target[free]) <= half[tau[free]] * (1 + 1e-12))
                both = free[:-1] & free[1:]
                gaps = lam[tau[:-1]] - lam[tau[1:]]
                step = (lam[0] - lam[-1]) / (S - 1)
                bound = half[tau[:-1]] + half[tau[1:]]
                assert np.all(np.abs(gaps - step)[both] <= bound[both] * (1 + 1e-12)), (S, np.abs(gaps - step)[both].max())
                if T >= 1000 and S <= 40:
                    # the forced part is the low end only, where one timestep moves lambda by more than a target spacing
                    assert both.sum() >= (S - 1) // 2, (S, both.sum())
                    assert free[S // 2:].all()
        with pytest.raises(ValueError):
            sampler_walk(ac, T + 1, walk)
        with pytest.raises(ValueError):
            sampler_walk(ac, 0, walk)
    with pytest.raises(ValueError):
        sampler_walk(ac, 2, 'cosine')


@pytest.mark.parametrize('walk', ['time', 'logsnr'])
@pytest.mark.parametrize('T,lo,hi', LINEAR)
def test_2m_tables_against_ddim(T, lo, hi, walk):
    """With r -> infinity (no curvature correction) 2M is DDIM: c1_2m + c3_2m == c1_ddim and c2_2m == c2_ddim on the same walk, to
    1e-12; a, b, sigma, level and tau are DDIM's own; the first step taken and the last have no history term."""
    from sr3_hip.diffusion import sampler_tables
    ac = _ac(T, lo, hi)
    for S in sorted({1, 2, 3, 7, 40, T} & set(range(1, T + 1))):
        dd = sampler_tables(ac, S, 0.0, kind='ddim', walk=walk)
        mm = sampler_tables(ac, S, 0.0, kind='dpmpp_2m', walk=walk)
        assert set(mm) == set(dd)
        for k in ('tau', 'a', 'b', 'sigma', 'level'):
            assert np.array_equal(mm[k], dd[k]), k
        assert not mm['sigma'].any()
        assert np.max(np.abs(mm['c1'] + mm['c3'] - dd['c1'])) <= 1e-12, (S, np.max(np.abs(mm['c1'] + mm['c3'] - dd['c1'])))
        assert np.max(np.abs(mm['c2'] - dd['c2'])) <= 1e-12
        assert mm['c3'][0] == 0.0 and mm['c3'][-1] == 0.0 and (mm['c1'][0], mm['c2'][0]) == (1.0, 0.0)
        if S <= 2:
            assert not mm['c3'].any()
        else:
            assert np.all(mm['c3'][1:-1] < 0.0)                   # D = x0 + (x0 - x0_prev) / (2r): the previous x0 enters negatively
        if S == 1:
            for k in dd:
                assert np.array_equal(mm[k], dd[k]), k
    for eta in (0.5, 1.0, 1e-9):
        with pytest.raises(ValueError):
            sampler_tables(ac, min(4, T), eta, kind='dpmpp_2m')
    with pytest.raises(ValueError):
        sampler_tables(ac, min(4, T), 0.0, kind='dpm-solver')
    with pytest.raises(ValueError):
        sampler_tables(ac, min(4, T), 0.0, walk='uniform')


def _toy_chain(ac, tab, v=0.09, x_T=0.7):
    """The scalar recurrence of the tail in float64 with the optimal denoiser of data ~ N(0, v), the clamp included: returns the final
    value and the largest |x0| met before the clamp."""
    x, hist, big = x_T, 0.0, 0.0
    for j in reversed(range(len(tab['tau']))):
        ab = ac[tab['tau'][j]]
        x0_true = np.sqrt(ab) * v / (ab * v + 1.0 - ab) * x           # E[x0 | x_t]
        eps = (x - np.sqrt(ab) * x0_true) / np.sqrt(1.0 - ab)
        x0 = tab['a'][j] * x - tab['b'][j] * eps
        big = max(big, abs(x0))
        x0 = min(max(x0, -1.0), 1.0)
        x = ((tab['c1'][j] * x0 + tab['c2'][j] * x) + tab['c3'][j] * hist) + tab['sigma'][j] * 0.0
        hist = x0
    return x, big


@pytest.mark.parametrize('S', [10, 20, 40])
@pytest.mark.parametrize('T,lo,hi', TABLE)
def test_2m_on_the_logsnr_walk_beats_ddim_fourfold_on_a_gaussian(T, lo, hi, S):
    """Data ~ N(0, 0.09), x_T = 0.7: the probability-flow ODE keeps x(t) proportional to sqrt(ac_t v + 1 - ac_t), and the expected
    output is the optimal denoiser applied to the ODE's value at timestep 0.  The error of dpmpp_2m on the log-SNR walk is at most a
    quarter of DDIM's on the time walk at the same S (measured margins: 10x and more), and the clamp never binds, so this compares
    the solvers."""
    from sr3_hip.diffusion import sampler_tables
    v, x_T = 0.09, 0.7
    ac = _ac(T, lo, hi)
    s = lambda a: np.sqrt(a * v + 1.0 - a)
    x_ode = x_T * s(ac[0]) / s(ac[-1])
    exact = np.sqrt(ac[0]) * v / (ac[0] * v + 1.0 - ac[0]) * x_ode
    got = {}
    for kind, walk in (('ddim', 'time'), ('dpmpp_2m', 'time'), ('ddim', 'logsnr'), ('dpmpp_2m', 'logsnr')):
        out, big = _toy_chain(ac, sampler_tables(ac, S, 0.0, kind=kind, walk=walk), v, x_T)
        got[kind, walk] = abs(out - exact)
        assert big < 1.0, (kind, walk, big)
    print('T = %d S = %d: ' % (T, S) + ', '.join('%s/%s %.1e' % (k + (e,)) for k, e in got.items()))
    assert got['dpmpp_2m', 'logsnr'] <= 0.25 * got['ddim', 'time'], got


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_config_surface(name):
    import model as Model
    from sr3_hip.diffusion import sampler_tables
    m = Model.create_model(opt_for(name, gpu=False))
    netG = m.netG
    s = SCHEDS[name]
    T = s['n_timestep']
    ac = _ac(T, s['linear_start'], s['linear_end'])
    keys = set(netG.state_dict().keys())
    assert netG.sampler is None and netG._sampler_c3 is None
    # plain DDIM: the dict it was, and no history table
    netG.set_sampler(3, 0.5)
    assert netG.sampler == dict(type='ddim', steps=3, eta=0.5) and netG._sampler_c3 is None
    netG.set_sampler(3, 0.5, kind='ddim', walk='time')
    assert netG.sampler == dict(type='ddim', steps=3, eta=0.5)
    # DDIM on the other walk
    netG._loop_cache['stale'] = object()
    netG.set_sampler(4, 0.0, walk='logsnr')
    assert netG.sampler == dict(type='ddim', steps=4, eta=0.0, walk='logsnr') and netG._sampler_c3 is None and netG._loop_cache == {}
    assert netG._sampler_tau.tolist() == sampler_tables(ac, 4, 0.0, walk='logsnr')['tau'].tolist()
    # the multistep solver: walk defaults to logsnr; the private tables are the float64 tables rounded once
    for walk in (None, 'logsnr', 'time'):
        netG.set_sampler(5, kind='dpmpp_2m', walk=walk)
        assert netG.sampler == dict(type='dpmpp_2m', steps=5, eta=0.0, walk=walk or 'logsnr')
        tab = sampler_tables(ac, 5, 0.0, kind='dpmpp_2m', walk=walk or 'logsnr')
        for k in ('a', 'b', 'c1', 'c2', 'c3', 'sigma', 'level'):
            assert torch.equal(getattr(netG, '_sampler_' + k), torch.tensor(tab[k], dtype=torch.float32)), k
        assert netG._sampler_tau.dtype == torch.int32 and netG._sampler_tau.tolist() == tab['tau'].tolist()
    assert set(netG.state_dict().keys()) == keys and netG.num_timesteps == T
    with pytest.raises(ValueError):
        netG.set_sampler(5, 0.5, kind='dpmpp_2m')
    with pytest.raises(ValueError):
        netG.set_sampler(5, walk='snr')
    with pytest.raises(NotImplementedError):
        netG.set_sampler(5, kind='dpm-solver')
    netG.set_sampler(None)
    assert netG.sampler is None and netG._sampler_c3 is None and netG._sampler_tau is None
    # the config route
    dev = torch.device('cpu')
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'dpmpp_2m', 'steps': 4}), dev)
    assert netG.sampler == dict(type='dpmpp_2m', steps=4, eta=0.0, walk='logsnr') and netG._sampler_c3.shape == (4,)
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'dpmpp_2m', 'steps': 4, 'walk': 'time', 'eta': 0}), dev)
    assert netG.sampler == dict(type='dpmpp_2m', steps=4, eta=0.0, walk='time')
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 4, 'eta': 0.25, 'walk': 'logsnr'}), dev)
    assert netG.sampler == dict(type='ddim', steps=4, eta=0.25, walk='logsnr')
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 4}), dev)
    assert netG.sampler == dict(type='ddim', steps=4, eta=0.0)
    with pytest.raises(ValueError):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'dpmpp_2m', 'steps': 4, 'eta': 0.5}), dev)
    with pytest.raises(ValueError):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'ddim', 'steps': 4, 'walk': 'snr'}), dev)
    with pytest.raises(NotImplementedError):
        netG.set_new_noise_schedule(dict(s, sampler={'type': 'unipc', 'steps': 4}), dev)
    netG.set_new_noise_schedule(dict(s), dev)
    assert netG.sampler is None and netG._sampler_c3 is None


def test_ddpm_tiling_under_the_multistep_sampler_is_refused():
    import model as Model
    netG = Model.create_model(opt_for('ddpm_tiny', gpu=False)).netG
    netG.set_tiling(16, 4)
    with pytest.raises(NotImplementedError):
        netG.set_sampler(4, kind='dpmpp_2m')
    assert netG.sampler is None
    netG.set_tiling(None)
    netG.set_sampler(4, kind='dpmpp_2m')
    with pytest.raises(NotImplementedError):
        netG.set_tiling(16, 4)
    assert netG.tiling is None
