#!/usr/bin/env python3
"""What noise conditioning augmentation with a level plane (GaussianDiffusion.set_cond_augment) costs, in two measurements on one box,
same tree:

(a) the 7-channel input conv at batch 16, 128 x 128, Cout = 32 NB for NB = 1..4: the MFMA form with fused GroupNorm statistics against
    the VALU kernel plus the stand-alone statistics pass.  Both are timed inside a forward (HIP events around every launch,
    sr3_unet_forward_profile) of a small plan whose first conv has that shape; the VALU leg needs a second build of the library,
    `SR3_BUILD_DIR=<dir> SR3_OUT=<lib> csrc/build.sh -DSR3_CONV_IN7_VALU`, passed as --valu-lib, and runs in a child process
    (SR3_LIBRARY).  Children of the two libraries alternate --reps times.
(b) the replayed reverse step of the BASELINE sampling config (SR3 16 -> 128, batch 16, the ancestral rule): the plain 6-channel model's
    fused step against the 7-channel model's (random weights; the conditioning tensor is built once per chain, so the step differs by
    the wider input conv alone), and the once-per-chain sr3_cond_augment_f32 call on its own.

Legs are interleaved --reps times after a warm-up round; best and median per leg.  One JSON line.
    python tools/condaug_probe.py [--valu-lib PATH] [--replays 100] [--reps 3]   (GPU box)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')
CONFIG = 'sr3_16_128'
CIN = 7


def conv_in_child(reps):
    """(a), one library: per NB the input conv's op time and the statistics op's behind it (0 where the conv fused them), ms, mean of reps"""
    import torch
    from sr3_hip import engine as E, lib as L
    lib = L.load()
    dev = torch.device('cuda', 0)
    B, S = 16, 128
    rec = {}
    for nb in (1, 2, 3, 4):
        cout = 32 * nb
        plan = E.Plan('sr3', CIN, 3, cout, 32, [1, 1, 1, 1], [], 1, S)      # (three halvings: the mid block's attention sees 16 x 16)
        arena = torch.randn(plan.param_floats, device=dev) * 0.02
        freq = plan.default_freq().to(dev)
        x, cond = torch.randn(B, 3, S, S, device=dev), torch.rand(B, CIN - 3, S, S, device=dev) * 2 - 1
        level, out = torch.full((B,), 0.5, device=dev), torch.empty(B, 3, S, S, device=dev)
        ws = E.Workspace()
        wsbuf, need = ws.get(plan, B, dev)
        derived = None
        dbytes = int(lib.sr3_plan_derived_bytes(plan.handle))
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if dbytes:
            derived = torch.empty((dbytes + 3) // 4, device=dev)
            L.check(lib.sr3_plan_bind_derived(plan.handle, L.ptr(derived), derived.numel() * 4))
            L.check(lib.sr3_plan_prepare_derived(plan.handle, L.ptr(arena), stream))
        max_ops = 4096
        ms, kind, fl, n = (C.c_float * max_ops)(), (C.c_int * max_ops)(), (C.c_double * max_ops)(), C.c_int()
        conv = stats = 0.0
        for r in range(reps + 1):                        # (r = 0 warms up)
            L.check(lib.sr3_unet_forward_profile(plan.handle, L.ptr(x), L.ptr(cond), CIN - 3, L.ptr(level), None, L.ptr(freq), L.ptr(arena),
                                                 L.ptr(wsbuf), need, L.ptr(out), B, stream, max_ops, ms, kind, fl, C.byref(n)))
            if r == 0:
                continue
            ops = plan.op_list(B)
            rows = [i for i in range(n.value) if int(kind[i]) != 59]      # (59: the entry of a split-K reduce behind its conv)
            assert len(rows) == len(ops) and ops[1]['kind'] == 20 and ops[1]['cin'] == CIN and ops[1]['cout'] == cout
            conv += ms[rows[1]] / reps
            if ops[2]['kind'] == 30:
                assert not ops[1]['fused_output_stats']
                stats += ms[rows[2]] / reps
            else:
                assert ops[1]['fused_output_stats']
        rec['nb%d' % nb] = dict(conv_ms=conv, stats_ms=stats, fused=bool(ops[1]['fused_output_stats']))
    print('CONV_IN ' + json.dumps(rec), flush=True)


def conv_in_legs(valu_lib, reps, inner_reps=5):
    legs = {'mfma_fused': None, 'valu_plus_stats': valu_lib}
    got = {k: {'nb%d' % nb: [] for nb in (1, 2, 3, 4)} for k in legs}
    fused = {}
    for _ in range(reps):
        for name, path in legs.items():
            env = dict(os.environ)
            if path is not None:
                env['SR3_LIBRARY'] = os.path.abspath(path)
            else:
                env.pop('SR3_LIBRARY', None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--conv-in-child', '--reps', str(inner_reps)], env=env,
                               stdout=subprocess.PIPE, check=True, timeout=300)
            line = [l for l in p.stdout.decode().splitlines() if l.startswith('CONV_IN ')][-1]
            for nb, r in json.loads(line[len('CONV_IN '):]).items():
                got[name][nb].append(r['conv_ms'] + r['stats_ms'])
                fused.setdefault(name, {})[nb] = r['fused']
    assert not any(fused['valu_plus_stats'].values()), fused
    rec = {name: {nb: {'best': min(v), 'median': statistics.median(v)} for nb, v in per.items()} for name, per in got.items()}
    rec['mfma_form_taken'] = fused['mfma_fused']         # (false: CONV_IN7_NB leaves that NB on the VALU kernel in this tree)
    return rec


def models():
    """the plain BASELINE model and its twin with a level plane (in_channel 7), random weights"""
    import torch
    import bench
    import model.networks as networks
    dev = torch.device('cuda', 0)
    out = {}
    for name in ('plain', 'level_channel'):
        torch.manual_seed(0)
        opt = bench.config_opt(CONFIG, n_timestep=2000, phase='val')
        if name == 'level_channel':
            opt['model']['unet']['in_channel'] = CIN
            opt['model']['diffusion']['cond_augment'] = {'max_level': 0.5, 'sample_level': 0.1, 'level_channel': True}
        netG = networks.define_G(opt).to(dev)
        netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
        netG.set_loss(dev)
        netG.show_progress = False
        out[name] = netG
    return out


def step_legs(replays, reps):
    import torch
    import bench
    dev = torch.device('cuda', 0)
    cfg = bench.CONFIGS[CONFIG]
    B, S = cfg['batch'], cfg['size']
    shape = (B, 3, S, S)
    cond = torch.rand(shape, device=dev) * 2 - 1
    nets = models()
    states = {}
    for name, netG in nets.items():
        netG.eval()
        aug = netG.cond_augment
        st = netG._loop_state(shape, (B, 4, S, S) if aug else shape, dev, cond_augment=aug is not None)
        netG.denoise_fn.ensure_derived()
        if aug:
            netG._augment_sampling_cond(st, aug, cond, None)
        else:
            st['cond'].copy_(cond)
        netG._capture(st)
        states[name] = st
    ms = {name: [] for name in states}
    ms['augment_call_once_per_chain'] = []
    for rep in range(reps + 1):                          # (rep 0 warms up)
        for name, st in states.items():
            st['img'].copy_(torch.randn(shape, device=dev))
            st['step'].fill_(replays - 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(replays):
                st['graph'].replay()
            e1.record()
            torch.cuda.synchronize()
            assert int(st['step'][1].item()) == -1 and bool(torch.isfinite(st['img']).all())
            if rep:
                ms[name].append(e0.elapsed_time(e1) / replays)
        netG, st = nets['level_channel'], states['level_channel']
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        netG._augment_sampling_cond(st, netG.cond_augment, cond, None)      # (the draw of the noise included)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms['augment_call_once_per_chain'].append(e0.elapsed_time(e1))
    return {name: {'best': min(v), 'median': statistics.median(v)} for name, v in ms.items()}, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--valu-lib', default=None, help='a build with -DSR3_CONV_IN7_VALU: adds (a)')
    ap.add_argument('--replays', type=int, default=100)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--conv-in-child', action='store_true')
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    if a.conv_in_child:
        return conv_in_child(a.reps)
    rec = {'what': 'noise conditioning augmentation', 'config': CONFIG, 'reps': a.reps}
    if a.valu_lib:                                       # children first: this process has not opened the GPU yet
        rec['conv_in_b16_128x128_ms'] = conv_in_legs(a.valu_lib, a.reps)
    rec['ms_per_step'], rec['batch'] = step_legs(a.replays, a.reps)
    rec['replays'] = a.replays
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
