"""What a compiled plan computes, bit for bit: equality with a recording, not closeness.

tests/golden/plan_run_bits.json holds, per case, the SHA-256 of the output bytes of one sr3_unet_forward, one sr3_reverse_step_hist (x,
eps_out and the two step counters) and one sr3_train_step (the loss bits and the gradient arena), recorded on an MI355X from the library
as it was while csrc/plan.hip bound the pointers and walked the launch list in one switch, run_forward took 21 positional parameters and
Builder::fold left its tables behind in cur_*.  The plan fingerprint pins WHICH kernels a plan launches; this pins what the driver binds
them to and in which order: a pointer, an offset, a fold table or a launch moved shows here as other bits.

Networks: sr3_seam and ddpm_tiny (tests/helpers.py) and W64 below -- 64 inner channels, so that the Winograd tiles, the plain GEMM kernel
and a split-K reduce that does the next GroupNorm's fold are all on one list that runs in well under a second (asserted below).  Batches
1 and 3, the native 16 x 16 and 16 x 24 (the training step off the native size under plan option train_geom), six option settings.
Inputs and weights come from seeded NumPy generators.  The training step runs with dropout 0.1: the mask is a counter-based hash.

Record again (on the GPU, only from a library whose bits are the wanted ones):  SR3_LIBRARY=/path/lib.so python tests/test_gpu_plan_bits.py [out.json]
(two passes; a case whose passes differ is not deterministic and is left out of the file: name it in NONDETERMINISTIC).
"""
import ctypes as C
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch                                                     # (before the library: it binds to the HIP runtime torch loaded)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plan_run_bits.json')
W64 = dict(variant='sr3', in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=[1, 2], attn_res=[8], res_blocks=1,
           image_size=16)
NETS = ('sr3_seam', 'ddpm_tiny', 'w64')
BATCHES = (1, 3)
GEOMETRIES = ((16, 16), (16, 24))
OPTIONS = (None, ('fold_fuse', 0), ('fuse_res', 0), ('fuse_stats', 0), ('winograd', 0), ('keep_all', 1))
CALLS = ('forward', 'step', 'train')
CONFIGS = [(n, b, g, o) for n in NETS for b in BATCHES for g in GEOMETRIES for o in OPTIONS]
NONDETERMINISTIC = ()      # case ids whose two recordings from the recorded library differed (never a default-option forward)
T_STEPS = 8


def desc(net):
    from helpers import DESCS
    return W64 if net == 'w64' else DESCS[net]


def config_id(c):
    net, batch, (h, w), opt = c
    return '%s-b%d-%dx%d-%s' % (net, batch, h, w, 'default' if opt is None else '%s=%d' % opt)


def make_plan(c):
    from sr3_hip import engine as E
    net, _, geo, opt = c
    d = desc(net)
    plan = E.Plan(d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'], d['attn_res'],
                  d['res_blocks'], d['image_size'])
    if opt is not None:
        plan.set_option(*opt)
    plan.set_geometry(*geo)
    return plan


_arenas = {}


def arena(net, plan):
    """the parameter arena of one network on the host, made once: weights N(0, 1 / fan_in), biases small, GroupNorm scales about 1"""
    if net not in _arenas:
        rng = np.random.default_rng(9100 + NETS.index(net))
        a = np.zeros(plan.param_floats, dtype=np.float32)
        for e in plan.table:
            n, shape = e['numel'], e['shape']
            if len(shape) >= 2:
                v = rng.standard_normal(n) / np.sqrt(n / shape[0])
            elif '.block.0.weight' in e['name'] or '.norm.weight' in e['name']:
                v = 1.0 + 0.1 * rng.standard_normal(n)
            else:
                v = 0.1 * rng.standard_normal(n)
            a[e['offset']:e['offset'] + n] = v.astype(np.float32)
        _arenas[net] = a
    return _arenas[net]


_inputs = {}


def inputs(net, batch, geo):
    """the host inputs of one (network, batch, geometry), made once and never changed"""
    key = (net, batch, geo)
    if key not in _inputs:
        (h, w), f32 = geo, np.float32
        rng = np.random.default_rng(77000 + 100 * NETS.index(net) + 10 * batch + w)
        img = lambda: rng.standard_normal((batch, 3, h, w)).astype(f32)
        t = dict(x=img(), cond=rng.uniform(-1, 1, (batch, 3, h, w)).astype(f32), z=img(), hr=rng.uniform(-1, 1, (batch, 3, h, w)).astype(f32),
                 hist=img(), level=rng.uniform(0.2, 0.95, batch).astype(f32), tstep=rng.integers(0, 2000, batch).astype(np.int64))
        t['ca'] = t['level'].copy()
        t['cb'] = np.sqrt(1 - t['level'].astype(np.float64) ** 2).astype(f32)
        # the step's tables, indexed by the counter t: x <- c1 x0 + c2 x + c3 hist + sigma z with x0 = a x - b eps
        t['level_table'] = np.linspace(0.99, 0.3, T_STEPS).astype(f32)
        for k, lo, hi in (('ta', 1.0, 1.5), ('tb', 0.1, 0.9), ('tc1', 0.1, 0.5), ('tc2', 0.4, 0.9), ('tsig', 0.01, 0.2), ('tc3', -0.2, 0.2)):
            t[k] = rng.uniform(lo, hi, T_STEPS).astype(f32)
        _inputs[key] = t
    return _inputs[key]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def aligned(nbytes, dev):
    buf = torch.zeros(nbytes + 256, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 256
    return buf[off:off + nbytes]


def run(c):
    """-> {call: digests} of one configuration on the device: a fresh plan, its derived buffer prepared, then the three calls"""
    import gpu_util as G
    from sr3_hip import lib as L
    net, B, (H, W), opt = c
    plan = make_plan(c)
    lib, h, dev = plan.lib, plan.handle, G.dev()
    sr3 = plan.variant == 'sr3'
    cc = 3 if sr3 else 0
    host = inputs(net, B, (H, W))
    t = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    params = torch.from_numpy(arena(net, plan)).to(dev)
    freq = plan.default_freq().to(dev)
    derived = aligned(max(int(lib.sr3_plan_derived_bytes(h)), 16), dev)
    L.check(lib.sr3_plan_bind_derived(h, L.ptr(derived), derived.numel()))
    L.check(lib.sr3_plan_prepare_derived(h, L.ptr(params), G.stream()))
    need = plan.workspace_bytes(B)
    ws = aligned(need, dev)
    cond = L.ptr(t['cond']) if sr3 else None
    nan = lambda *shape: torch.full(shape, float('nan'), device=dev)
    got = {}

    eps = nan(B, 3, H, W)
    L.check(lib.sr3_unet_forward(h, L.ptr(t['x']), cond, cc, L.ptr(t['level']) if sr3 else None, None if sr3 else L.ptr(t['tstep']), L.ptr(freq),
                                 None, None, L.ptr(params), L.ptr(ws), need, L.ptr(eps), B, G.stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eps).all()), 'an element of eps was not written, or the forward overflowed'
    got['forward'] = {'eps': sha(eps)}

    x, hist, eps = t['x'].clone(), t['hist'].clone(), nan(B, 3, H, W)
    step2 = torch.tensor([0, 5], dtype=torch.int32, device=dev)
    L.check(lib.sr3_reverse_step_hist(h, L.ptr(x), cond, cc, L.ptr(freq), L.ptr(t['level_table']), L.ptr(step2), L.ptr(params), L.ptr(ws), need,
                                      L.ptr(t['z']), L.ptr(t['ta']), L.ptr(t['tb']), L.ptr(t['tc1']), L.ptr(t['tc2']), L.ptr(t['tsig']), 1, L.ptr(eps),
                                      B, G.stream(), None, L.ptr(t['tc3']), L.ptr(hist)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(eps).all())
    got['step'] = {'x': sha(x), 'eps': sha(eps), 'hist': sha(hist), 'step2': step2.tolist()}

    if (H, W) != (plan.image_size, plan.image_size):
        plan.set_option('train_geom', 1)      # (no effect on what ran above; off the native size the training step needs it)
    tneed = int(lib.sr3_train_workspace_bytes(h, B, cc))
    assert tneed > 0, lib.sr3_last_error()
    tws = aligned(tneed, dev)
    grads, loss = nan(plan.param_floats), nan(1)
    L.check(lib.sr3_train_step(h, L.ptr(t['hr']), cond, cc, L.ptr(t['z']), L.ptr(t['ca']), L.ptr(t['cb']), L.ptr(t['level']) if sr3 else None,
                               None if sr3 else L.ptr(t['tstep']), L.ptr(freq), L.ptr(params), L.ptr(grads), L.ptr(tws), tneed, L.ptr(loss),
                               C.c_float(1.0 / (B * 3 * H * W)), C.c_float(0.1), C.c_uint(20241021), 0, None, None, B, G.stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grads).all()), 'a gradient was not written'
    got['train'] = {'loss': struct.unpack('<I', struct.pack('<f', float(loss)))[0], 'grads': sha(grads)}
    return got


def case_ids():
    return ['%s/%s' % (config_id(c), call) for c in CONFIGS for call in CALLS]


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted(set(case_ids()) - set(NONDETERMINISTIC))
    assert not [k for k in NONDETERMINISTIC if k.endswith('-default/forward')], 'a default-option forward has to be deterministic'


def test_w64_has_the_kernels_it_is_here_for():
    """Winograd tiles, the plain GEMM kernel and a split-K conv are on W64's list, and fold_fuse = 0 adds fold launches: some fold of the
    default list is done by another op's last kernel (a split-K reduce or a statistics pass)."""
    for B in BATCHES:
        plan = make_plan(('w64', B, (16, 16), None))
        convs = [o for o in plan.op_list(B) if o['kind'] == 50]
        assert any(o['tile_cfg'] in (12, 13) for o in convs) and any(o['tile_cfg'] == 22 for o in convs), sorted({o['tile_cfg'] for o in convs})
        assert any(o['ksplit'] > 1 and o['fused_output_stats'] for o in convs), 'no split-K conv whose reduce writes statistics'
        folds = lambda p: sum(o['kind'] == 40 for o in p.op_list(B))
        assert folds(make_plan(('w64', B, (16, 16), ('fold_fuse', 0)))) > folds(plan)


@pytest.mark.parametrize('c', CONFIGS, ids=config_id)
def test_plan_bits_are_the_recorded_ones(recorded, c):
    got = run(c)
    for call in CALLS:
        cid = '%s/%s' % (config_id(c), call)
        print('%s: got %s, recorded %s' % (cid, got[call], recorded.get(cid)))
    for call in CALLS:
        cid = '%s/%s' % (config_id(c), call)
        if cid not in NONDETERMINISTIC:
            assert got[call] == recorded[cid], cid


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    sys.path[:0] = [root, os.path.join(root, 'image-super-resolution-via-iterative-refinement_amd'), here]
    from sr3_hip import lib as L
    L.load()
    passes = []
    for _ in range(2):
        out = {}
        for c in CONFIGS:
            got = run(c)
            out.update(('%s/%s' % (config_id(c), call), got[call]) for call in CALLS)
        passes.append(out)
    differ = sorted(k for k in passes[0] if passes[0][k] != passes[1][k])
    print('cases whose two passes differ (left out): %s' % differ)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, 'w') as f:
        json.dump({k: v for k, v in passes[0].items() if k not in differ}, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d cases from %s into %s' % (len(passes[0]) - len(differ), L.LIB_PATH, path))
