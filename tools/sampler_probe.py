#!/usr/bin/env python3
"""What a replayed reverse step costs under a sampler (GaussianDiffusion.set_sampler) next to the ancestral step: the
captured step graph of the BASELINE config at its batch, replayed --replays times per leg and timed with HIP events -- the ancestral
loop, the DDIM sampler at eta = 0 (no RNG node, no z read) and at eta = 0.5, and the multistep solver dpmpp_2m (eta = 0, plus one read
and one write of the image-sized history in the output conv's epilogue) -- legs interleaved --reps times, best and median per leg; then
the wall time of whole `super_resolution` chains of --chain steps (capture excluded).  --consistency R adds a leg: dpmpp_2m with the
block-mean projection of set_consistency(R) in its tail (three graph nodes -- forward with eps stored, counter copy, sr3_consistent_step
-- in place of the fused step), next to the dpmpp_2m leg in every round.  --guidance SCALE --threshold MODE (either may be given more
than once, paired in order) adds a leg per pair: dpmpp_2m under set_guidance(SCALE, MODE) -- one forward (scale 1) or two, each with its
output stored, then sr3_guided_step in place of the fused step; --no-chains skips the whole-chain timings.  --backprojection S
--bp-iterations K (K may be given more than once) adds a leg per K: dpmpp_2m under set_backprojection(S, K) -- the forward with eps
stored, then sr3_backproject_step (2 + 3 K launches) in place of the fused step.
    python tools/sampler_probe.py [--config sr3_16_128] [--replays 200] [--reps 3] [--chain 100] [--consistency 8]
                                  [--guidance 1.5 --threshold dynamic] [--backprojection 8 --bp-iterations 1 --bp-iterations 2]   (GPU box)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='sr3_16_128')
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--chain', type=int, default=100)
    ap.add_argument('--consistency', type=int, default=0, metavar='BLOCK', help='add the dpmpp_2m leg with set_consistency(BLOCK)')
    ap.add_argument('--guidance', type=float, action='append', default=[], metavar='SCALE', help='add a dpmpp_2m leg with set_guidance(SCALE, MODE)')
    ap.add_argument('--threshold', action='append', default=[], metavar='MODE', help='static (default) | none | dynamic, one per --guidance')
    ap.add_argument('--percentile', type=float, default=0.995)
    ap.add_argument('--backprojection', type=int, default=0, metavar='SCALE', help='add dpmpp_2m legs with set_backprojection(SCALE, K)')
    ap.add_argument('--bp-iterations', type=int, action='append', default=[], metavar='K', help='one leg per K (default: 1)')
    ap.add_argument('--no-chains', action='store_true', help='time the replayed steps only')
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import model.networks as networks
    cfg = bench.CONFIGS[a.config]
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    opt = bench.config_opt(a.config, n_timestep=2000)
    netG = networks.define_G(opt).to(dev)
    netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
    netG.eval()
    netG.show_progress = False
    netG.max_cached_loops = 4
    B, S = cfg['batch'], cfg['size']
    shape = (B, 3, S, S)
    cond = (torch.rand(shape, device=dev) * 2 - 1) if cfg['conditional'] else None
    N = a.replays
    legs = {'ancestral': dict(steps=None), 'ddim_eta0': dict(steps=N, eta=0.0), 'ddim_eta0.5': dict(steps=N, eta=0.5),
            'dpmpp_2m': dict(steps=N, kind='dpmpp_2m')}
    if a.consistency:
        assert cond is not None, '--consistency needs a conditional config'
        legs['dpmpp_2m_consistency'] = dict(steps=N, kind='dpmpp_2m', consistency=a.consistency)
    for i, scale in enumerate(a.guidance):
        assert cond is not None, '--guidance needs a conditional config'
        mode = a.threshold[i] if i < len(a.threshold) else 'static'
        legs['dpmpp_2m_guidance%g_%s' % (scale, mode)] = dict(steps=N, kind='dpmpp_2m', guidance=(scale, mode, a.percentile))
    if a.backprojection:
        assert cond is not None, '--backprojection needs a conditional config'
        for k in (a.bp_iterations or [1]):
            legs['dpmpp_2m_backprojection%d_K%d' % (a.backprojection, k)] = dict(steps=N, kind='dpmpp_2m', backprojection=(a.backprojection, k))
    states = {}
    for name, spec in legs.items():                      # one captured graph per leg, all alive at once
        spec = dict(spec)
        netG.set_guidance(None)
        netG.set_backprojection(None)
        netG.set_consistency(spec.pop('consistency', None))
        gd = spec.pop('guidance', None)
        bp = spec.pop('backprojection', None)
        netG.set_sampler(**spec)
        if gd is not None:
            netG.set_guidance(*gd)
        if bp is not None:
            netG.set_backprojection(*bp)
        st = netG._loop_state(shape, shape if cond is not None else None, dev, consistency=netG.consistency, guidance=netG.guidance,
                              backprojection=netG.backprojection)
        netG.denoise_fn.ensure_derived()
        if cond is not None:
            st['cond'].copy_(cond)
        if netG.consistency is not None:
            from sr3_hip.diffusion import block_means
            st['ymean'].copy_(block_means(cond, a.consistency))
        if netG.backprojection is not None:
            from sr3_hip.diffusion import resample_f32
            st['y_lr'].copy_(resample_f32(cond, tuple(st['y_lr'].shape[2:]), tables=st['bp_down']))
        netG._capture(st)
        states[name] = st
    ms = {name: [] for name in legs}
    for rep in range(a.reps + 1):                        # (rep 0 warms up)
        for name, st in states.items():
            st['img'].copy_(torch.randn(shape, device=dev))
            if st.get('hist') is not None:
                st['hist'].zero_()
            st['step'].fill_(N - 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(N):
                st['graph'].replay()
            e1.record()
            torch.cuda.synchronize()
            assert int(st['step'][1].item()) == -1 and bool(torch.isfinite(st['img']).all())
            if rep:
                ms[name].append(e0.elapsed_time(e1) / N)
    rec = {'what': 'sampler step', 'config': a.config, 'batch': B, 'replays': N, 'reps': a.reps}
    for name in legs:
        rec['ms_per_step_' + name] = {'best': min(ms[name]), 'median': statistics.median(ms[name])}
    netG.set_consistency(None)
    netG.set_guidance(None)
    netG.set_backprojection(None)
    if a.no_chains:
        print(json.dumps(rec))
        return
    arg = cond if cond is not None else shape
    for kind, eta in (('ddim', 0.0), ('ddim', 0.5), ('dpmpp_2m', 0.0)):
        netG.set_sampler(a.chain, eta, kind=kind)
        netG.p_sample_loop(arg)                          # capture + one chain (warm)
        torch.cuda.synchronize()
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = netG.p_sample_loop(arg)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        assert bool(torch.isfinite(out).all())
        rec['chain_%d_steps_%seta%g_wall_s' % (a.chain, '' if kind == 'ddim' else kind + '_', eta)] = {'best': min(walls), 'median': statistics.median(walls)}
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
