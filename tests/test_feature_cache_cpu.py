"""Feature-cached sampling without a device: the plan option and its shallow launch list, the cache size, the refresh schedule, the
config key, the refusals, the loop-state key -- and the oracle restatement the GPU tests compare against."""
import copy
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import DESCS, SCHEDS, load_golden, opt_for          # noqa: E402

B = 2
# what the two tiny plans compile to at batch 2 without the option: (ops, workspace bytes)
PARENT = {'sr3_tiny': (75, 131840), 'ddpm_tiny': (84, 149760)}
DEPTHS = [('sr3_tiny', 1), ('sr3_tiny', 2), ('ddpm_tiny', 1), ('ddpm_tiny', 2), ('ddpm_tiny', 3)]


def plan_of(name):
    from sr3_hip import engine as E
    d = DESCS[name]
    return E.Plan(d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'], d['attn_res'],
                  d['res_blocks'], d['image_size'])


def shape_of(o):
    return tuple(o[k] for k in ('kind', 'ksize', 'stride', 'upsample', 'cin', 'cout', 'h_out', 'w_out'))


# ---- the plan ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_option_off_is_the_parent_plan(name):
    from sr3_hip import lib as L
    plan, fresh = plan_of(name), plan_of(name)
    ops, ws = fresh.op_list(B), fresh.workspace_bytes(B)
    assert (len(ops), ws) == PARENT[name]
    assert plan.feature_cache_bytes(B) == 0 and plan.generation == 0
    with pytest.raises(L.Sr3Error, match='feat_cache is off'):
        plan.shallow_op_list(B)
    plan.set_option('feat_cache', 1)
    assert plan.generation == 1 and plan.options['feat_cache'] == 1 and plan.feature_cache_bytes(B) > 0
    assert plan.op_list(B) == ops, 'the full list of a plan under the option is not the plain list'
    plan.set_option('feat_cache', 0)
    assert plan.generation == 2 and plan.feature_cache_bytes(B) == 0
    assert plan.op_list(B) == ops and plan.workspace_bytes(B) == ws
    # not a key of sr3_plan_set_option: the option has an entry of its own
    assert plan.lib.sr3_plan_set_option(plan.handle, b'feat_cache', 1) < 0 and plan.lib.sr3_last_error().decode().startswith('unknown option')


@pytest.mark.parametrize('name,depth', DEPTHS)
def test_shallow_list(name, depth):
    plan = plan_of(name)
    full = [shape_of(o) for o in plan.op_list(B)]
    plan.set_option('feat_cache', depth)
    shallow = [shape_of(o) for o in plan.shallow_op_list(B)]
    assert shallow[0][0] == 10 and shallow[-1][0] == 70 and len(shallow) < len(full)
    it = iter(full)
    assert all(any(s == f for f in it) for s in shallow), 'the shallow list is not an ordered subsequence of the full one'
    # the convs: one input conv, and per res block conv1, conv2 and -- where the channel count changes -- res_conv; no attention at 16 x 16
    d = DESCS[name]
    inner = d['inner_channel']
    convs = [s for s in shallow if s[0] == 50]
    assert sum(1 for s in shallow if s[0] == 20) == 1 and not any(s[0] == 60 for s in shallow)
    assert all(s[6:] == (16, 16) and s[5] == inner for s in convs)
    downs = [s for s in convs if s[4] == inner]
    ups = [s for s in convs if s[4] > inner]
    assert len(downs) == 2 * (depth - 1) + depth and len(ups) == 2 * depth      # (+ depth: conv2 of every up block reads Cout channels)
    assert plan.workspace_bytes(B) > 0


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_cache_holds_at_least_the_branch_tensor(name):
    import feature_cache_ref as R
    from oracle import sr3_oracle as O
    desc = DESCS[name]
    topo = O.unet_topology(desc)
    for depth in range(1, desc['res_blocks'] + 2):
        plan = plan_of(name)
        plan.set_option('feat_cache', depth)
        first = topo['ups'][len(topo['ups']) - depth]
        branch_channels = first['cin'] - first['skip']
        assert R.branch_name(desc, depth) in [l['name'] for l in topo['ups'] + topo['mid']]
        assert plan.feature_cache_bytes(B) >= B * branch_channels * 16 * 16 * 4
        assert plan.feature_cache_bytes(2 * B) >= 2 * B * branch_channels * 16 * 16 * 4


@pytest.mark.parametrize('name', ['sr3_tiny', 'ddpm_tiny'])
def test_depth_outside_the_top_level_is_refused(name):
    from sr3_hip import lib as L
    plan = plan_of(name)
    rb = DESCS[name]['res_blocks']
    for bad in (rb + 2, -1):
        with pytest.raises(L.Sr3Error, match=r'error -2: feat_cache %d: .*1 \.\. %d' % (bad, rb + 1)):
            plan.set_option('feat_cache', bad)
    assert plan.generation == 0 and 'feat_cache' not in plan.options
    netG = build(opt_for(name, phase='val', gpu=False))
    for bad in (0, rb + 2):
        with pytest.raises(ValueError, match='feature_cache depth'):
            netG.set_feature_cache(3, depth=bad)
    assert netG.feature_cache is None and netG.denoise_fn.plan.generation == 0


# ---- the schedule --------------------------------------------------------------------------------------------------------------

def test_refresh_schedule():
    from sr3_hip.schedules import feature_cache_refresh as f
    assert [f(k, 8, 3) for k in range(8)] == [True, False, False, True, False, False, True, False]
    assert [f(k, 8, 3, 2) for k in range(8)] == [True, False, False, True, False, False, True, True]
    assert [f(k, 7, 5, 3) for k in range(7)] == [True, False, False, False, True, True, True]
    assert all(f(k, 8, 1) for k in range(8)) and all(f(k, 8, 4, 8) for k in range(8))
    assert [f(k, 5, 10) for k in range(5)] == [True] + [False] * 4
    for n in (1, 2, 9):
        for interval in (1, 2, 3, 5, 10):
            assert f(0, n, interval)                         # a chain's first step always refills the cache
    for bad in ((8, 8, 3), (-1, 8, 3), (0, 8, 0), (0, 8, 3, -1)):
        with pytest.raises(ValueError):
            f(*bad)


# ---- configuration -------------------------------------------------------------------------------------------------------------

def build(opt):
    from model import networks
    netG = networks.define_G(copy.deepcopy(opt))
    netG.set_new_noise_schedule(opt['model']['beta_schedule'][opt['phase']], torch.device('cpu'))
    return netG


def test_config_key_and_setter():
    from sr3_hip.schedules import parse_feature_cache
    opt = opt_for('ddpm_tiny', phase='val', gpu=False)
    netG = build(opt)
    plan = netG.denoise_fn.plan
    assert netG.feature_cache is None and plan.generation == 0 and 'feat_cache' not in plan.options      # absent: nothing is touched
    s = SCHEDS['ddpm_tiny']
    cpu = torch.device('cpu')
    netG.set_new_noise_schedule(dict(s, feature_cache={'interval': 3}), cpu)
    assert netG.feature_cache == dict(interval=3, depth=1, full_last=0) and plan.options['feat_cache'] == 1
    netG.set_new_noise_schedule(dict(s, sampler={'type': 'dpmpp_2m', 'steps': 4}, feature_cache={'interval': 2, 'depth': 3, 'full_last': 1}), cpu)
    assert netG.feature_cache == dict(interval=2, depth=3, full_last=1) and plan.options['feat_cache'] == 3
    gen = plan.generation
    netG.set_feature_cache(5, depth=3)                       # the same depth: the launch list stays
    assert plan.generation == gen and netG.feature_cache == dict(interval=5, depth=3, full_last=0)
    netG.set_new_noise_schedule(dict(s), cpu)                # the next phase's block has no key: off
    assert netG.feature_cache is None and plan.options['feat_cache'] == 0 and plan.feature_cache_bytes(B) == 0
    netG.set_feature_cache(2)
    netG.set_feature_cache(None)
    assert netG.feature_cache is None and plan.options['feat_cache'] == 0
    assert parse_feature_cache(None) == dict(interval=None)
    for bad, msg in (({'depth': 1}, '"interval" is required'), ({'interval': 2, 'every': 3}, 'unknown key'), (3, 'a dict')):
        with pytest.raises(ValueError, match=msg):
            parse_feature_cache(bad)
    for kw in (dict(interval=0), dict(interval=2.5), dict(interval=True), dict(interval=2, full_last=-1), dict(interval=2, depth='1')):
        with pytest.raises(ValueError, match='feature_cache'):
            netG.set_feature_cache(**kw)


FC = dict(interval=3)
# (what switches the other setting on, what switches it off, the words the refusal names it by)
OTHERS = [
    (lambda n: n.set_tiling(16, 4), lambda n: n.set_tiling(None), 'feature_cache with tiling'),
    (lambda n: n.set_consistency(4), lambda n: n.set_consistency(None), 'feature_cache with consistency'),
    (lambda n: n.set_guidance(1.5), lambda n: n.set_guidance(None), 'feature_cache with guidance.*two caches'),
    (lambda n: n.set_backprojection(4), lambda n: n.set_backprojection(None), 'feature_cache with backprojection'),
    (lambda n: n.set_restore('gray'), lambda n: n.set_restore(None), 'feature_cache with restore'),
    (lambda n: n.set_restore('gray', travel={'length': 2, 'repeats': 2}), lambda n: n.set_restore(None), 'feature_cache with restore.*travelled walk'),
]


@pytest.mark.parametrize('on,off,words', OTHERS)
def test_refusals_from_both_orders(on, off, words):
    netG = build(opt_for('sr3_tiny', phase='val', gpu=False))
    netG.set_feature_cache(**FC)
    with pytest.raises(NotImplementedError, match=words):
        on(netG)
    netG.set_feature_cache(None)
    on(netG)
    with pytest.raises(NotImplementedError, match=words):
        netG.set_feature_cache(**FC)
    assert netG.feature_cache is None and netG.denoise_fn.plan.options.get('feat_cache', 0) == 0
    off(netG)
    netG.set_feature_cache(**FC)
    # ... and from the config, where both keys stand in one block
    assert netG.feature_cache == dict(interval=3, depth=1, full_last=0)


def test_self_conditioning_is_refused_from_both_orders():
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    opt['model']['unet']['in_channel'] = 9
    netG = build(opt)
    netG.set_feature_cache(**FC)
    with pytest.raises(NotImplementedError, match='feature_cache with self-conditioning'):
        netG.set_self_condition(0.5)
    netG.set_feature_cache(None)
    netG.set_self_condition(0.5)
    with pytest.raises(NotImplementedError, match='feature_cache with self-conditioning'):
        netG.set_feature_cache(**FC)


def test_learned_variance_ancestral_tail_is_refused_from_both_orders():
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    opt['model']['unet']['out_channel'] = 6
    opt['model']['diffusion']['learned_variance'] = {'lambda': 0.001}
    netG = build(opt)
    assert netG.sampler['type'] == 'ancestral'
    with pytest.raises(NotImplementedError, match='feature_cache with the learned-variance ancestral sampler'):
        netG.set_feature_cache(**FC)
    netG.set_sampler(4, 0.0, kind='ddim')                    # on the prediction rows, with the table sigma: the fused step
    netG.set_feature_cache(**FC)
    with pytest.raises(NotImplementedError, match='feature_cache with the learned-variance ancestral sampler'):
        netG.set_sampler(8, kind='ancestral')
    assert netG.sampler['type'] == 'ddim'


def test_cond_augment_rides_along_and_the_loops_that_do_not():
    netG = build(opt_for('sr3_tiny', phase='val', gpu=False))
    netG.set_feature_cache(**FC)
    netG.set_cond_augment(0.3, 0.1, level_channel=False)
    assert netG.cond_augment is not None and netG.feature_cache is not None
    netG.set_cond_augment(None)
    with pytest.raises(NotImplementedError, match='calc_bpd_loop with feature_cache'):
        netG.calc_bpd_loop({'HR': torch.zeros(1, 3, 16, 16), 'SR': torch.zeros(1, 3, 16, 16)})
    with pytest.raises(NotImplementedError, match='feature_cache with tiling'):      # the tiling p_sample_loop_tiled hands the check, too
        netG._check_settings(tiling=dict(tile=(16, 16), overlap=4, batch=None))


def test_distillation_is_refused_from_both_orders():
    from sr3_hip import distill as DS
    opt = opt_for('sr3_tiny', phase='val', gpu=False)
    student, teacher = build(opt), build(opt)
    teacher.set_feature_cache(**FC)
    with pytest.raises(NotImplementedError, match='feature_cache with train.distill.*teacher'):
        DS.Distiller(student, teacher, 2)
    teacher.set_feature_cache(None)
    student.set_feature_cache(**FC)
    with pytest.raises(NotImplementedError, match='feature_cache with train.distill.*student'):
        DS.Distiller(student, teacher, 2)
    # switched on behind a Distiller: refused at the step
    student.set_feature_cache(None)
    dist = object.__new__(DS.Distiller)
    dist.student, dist.teacher = student, teacher
    student.set_feature_cache(**FC)
    with pytest.raises(NotImplementedError, match='feature_cache with train.distill'):
        dist.step({'HR': torch.zeros(1, 3, 16, 16), 'SR': torch.zeros(1, 3, 16, 16)})


# ---- the loop state ------------------------------------------------------------------------------------------------------------

def test_loop_key_gains_a_component_only_with_the_key():
    netG = build(opt_for('sr3_tiny', phase='val', gpu=False))
    seen = []

    class Stop(Exception):
        pass

    class Cache(dict):
        def get(self, key, default=None):
            seen.append(key)
            raise Stop

    def key():
        netG._loop_cache = Cache()
        with pytest.raises(Stop):
            netG._loop_state((2, 3, 16, 16), (2, 3, 16, 16), torch.device('cpu'))
        netG._loop_cache = {}
        return seen[-1]
    plain = key()
    assert len(plain) == 13 and plain[-1] is None and plain[-2] is None and plain[-3] is None and plain[-4] is None      # the tiling entry last
    netG.set_feature_cache(3, depth=2, full_last=1)
    with_fc = key()
    gen = netG.denoise_fn.plan.generation
    assert gen == 1 and with_fc[6] == gen and plain[6] == 0
    assert with_fc[:6] == plain[:6] and with_fc[7:13] == plain[7:] and with_fc[13:] == (('feature_cache', 2),)
    netG.set_feature_cache(None)
    assert key()[:6] == plain[:6] and len(key()) == 13


# ---- the oracle restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,depth', DEPTHS)
def test_reference_is_the_forward_at_the_refresh_point_and_differs_behind_it(name, depth):
    """cached at A on A's own branch tensor is the full forward at A (the same arithmetic, cut and rejoined); at an independent B it
    stands far from the full forward at B -- the gap the GPU test's staleness check needs (ten step tolerances)."""
    import feature_cache_ref as R
    _, sd = load_golden(name)
    xa, ta, xb, tb = R.inputs(DESCS[name])
    full_a, cached_a, again = R.cached_forward(sd, DESCS[name], depth, xa, ta, xa, ta)
    assert torch.equal(full_a, again) and (cached_a - full_a).abs().max().item() <= 1e-6 * max(1.0, full_a.abs().max().item())
    _, cached_b, full_b = R.cached_forward(sd, DESCS[name], depth, xa, ta, xb, tb)
    gap = (cached_b - full_b).abs().max().item()
    assert gap > 10 * R.TOL * max(1.0, full_b.abs().max().item()), gap
