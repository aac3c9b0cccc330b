#!/usr/bin/env python3
"""What feature-cached sampling (GaussianDiffusion.set_feature_cache) buys and costs, measured: per config (the BASELINE C2 network,
SR3 16 -> 128 at batch 16, and C5, DDPM-128 at batch 32; random weights of seed 0, as bench.py builds them)
  * the replayed step graph in ms: the full step without the option, the full step of a plan under the option at depth 1 / 2 / 3 (what
    the option adds to a full step: the branch tensor's producer writes into the cache), the cached step at each depth;
  * for interval in 2, 3, 5, 10 (depth --depth, default 1): the wall time per step of a whole --chain step ancestral chain (capture
    excluded) and the max-abs and RMS distance of its final image from the uncached chain on the same seed and x_T; interval 3 once
    more with full_last = a tenth of the chain.
No trained checkpoint is on the machines: the distances are those of random weights and bound NOTHING about image quality; no target
is set for them.  They show that the cached chain is a different chain, how far apart on this network, and that it stays finite.
    python tools/feature_cache_probe.py [--configs sr3_16_128 ddpm_128] [--replays 50] [--reps 3] [--chain 200] [--out profiles/feature_cache_probe.json]   (GPU box)"""
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
    ap.add_argument('--configs', nargs='+', default=['sr3_16_128', 'ddpm_128'])
    ap.add_argument('--replays', type=int, default=50)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--chain', type=int, default=200)
    ap.add_argument('--depth', type=int, default=1, help='the depth the chains run at')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'feature_cache_probe.json'))
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import model.networks as networks
    dev = torch.device('cuda', 0)
    T = max(a.chain, a.replays + 8)

    def replay_ms(st, slot):
        """best and median over --reps of the mean replay time of st[slot] over --replays replays, in ms"""
        ms = []
        for _ in range(a.reps):
            st['step'].fill_(T - 1)
            for _ in range(3):
                st[slot].replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                st[slot].replay()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.replays)
        return dict(best=round(min(ms), 4), median=round(statistics.median(ms), 4))

    record = {'what': __doc__.split('\n')[0], 'replays': a.replays, 'reps': a.reps, 'chain_steps': a.chain, 'chain_depth': a.depth,
              'note': 'random weights (seed 0): the distances bound nothing about image quality, and no target is set for them',
              'device': torch.cuda.get_device_name(0), 'configs': {}}
    for name in a.configs:
        cfg = bench.CONFIGS[name]
        torch.manual_seed(0)
        opt = bench.config_opt(name, n_timestep=T)
        netG = networks.define_G(opt).to(dev)
        netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
        netG.eval()
        netG.show_progress = False
        B, S = cfg['batch'], cfg['size']
        shape = (B, 3, S, S)
        cshape = shape if cfg['conditional'] else None
        g = torch.Generator(device=dev).manual_seed(1)
        cond = (torch.rand(shape, device=dev, generator=g) * 2 - 1) if cfg['conditional'] else None
        x_T = torch.randn(shape, device=dev, generator=g)
        plan = netG.denoise_fn.plan
        out = {'batch': B, 'size': S, 'ops_full': plan.num_ops(B), 'steps': {}, 'chains': {}}

        def state():
            st = netG._loop_state(shape, cshape, dev)
            if cond is not None:
                st['cond'].copy_(cond)
            st['img'].copy_(x_T)
            st['step'].fill_(T - 1)
            netG.denoise_fn.ensure_derived()
            return st

        st = state()
        netG._capture(st)
        out['steps']['full_uncached'] = replay_ms(st, 'graph')
        for depth in range(1, min(3, plan.desc.res_blocks + 1) + 1):
            netG.set_feature_cache(2, depth=depth)
            st = state()
            st['refresh'] = True
            netG._capture(st)
            st['refresh'] = False
            netG._capture(st, None, 'graph_cached')
            out['steps']['depth%d' % depth] = dict(full=replay_ms(st, 'graph'), cached=replay_ms(st, 'graph_cached'),
                                                 ops_cached=len(plan.shallow_op_list(B)), cache_bytes=plan.feature_cache_bytes(B),
                                                 workspace_bytes=plan.workspace_bytes(B))
        netG.set_feature_cache(None)

        def chain():
            """(final image, wall ms per step) of one whole chain; the first call of a setting captures, the second is timed"""
            arg = cond if cond is not None else shape
            for timed in (False, True):
                torch.manual_seed(2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                img = netG.p_sample_loop(arg, continous=False, x_T=x_T)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            return img.clone(), 1e3 * dt / a.chain

        netG.set_new_noise_schedule(bench.config_opt(name, n_timestep=a.chain)['model']['beta_schedule']['val'], dev)
        base, ms = chain()
        out['chains']['uncached'] = dict(ms_per_step=round(ms, 4))
        # (interval 3 once more with the last tenth of the chain run whole: what full_last buys in distance and costs in time)
        for interval, full_last in ((2, 0), (3, 0), (5, 0), (10, 0), (3, a.chain // 10)):
            netG.set_feature_cache(interval, depth=a.depth, full_last=full_last)
            img, ms = chain()
            diff = (img.double() - base.double())
            out['chains']['interval%d' % interval + ('_full_last%d' % full_last if full_last else '')] = dict(
                ms_per_step=round(ms, 4), speedup=round(out['chains']['uncached']['ms_per_step'] / ms, 3),
                max_abs=float(diff.abs().max()), rms=float(diff.pow(2).mean().sqrt()), finite=bool(torch.isfinite(img).all()),
                base_rms=float(base.double().pow(2).mean().sqrt()))
        netG.set_feature_cache(None)
        record['configs'][name] = out
        print(name, json.dumps(out), flush=True)
        del netG, st
        torch.cuda.empty_cache()
    with open(a.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
