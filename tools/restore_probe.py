#!/usr/bin/env python3
"""What a restoring reverse step (GaussianDiffusion.set_restore) costs next to the consistency step: per config (the BASELINE shapes
sr3_16_128 at batch 16 and ddpm_128 at batch 32)

  tails   the entries alone through the C ABI on tensors of the config's image shape, --calls calls per leg between two HIP events:
          sr3_consistent_step (block 8), sr3_restore_step with a one-plane mask, a per-channel mask and the gray operator, each with z,
          no history (the DDIM / ancestral form), and sr3_travel_back_f32.  Every leg includes its own step_copy launch.  Next to the
          time: the bytes the leg has to move (x read and written, eps, z and the target / mask read once) and the rate that makes.
  steps   the captured step graph -- forward with eps stored, then the tail -- replayed --replays times under DDIM eta 0: the fused
          step, consistency (conditional configs), restore mask, restore gray.

Legs are interleaved --reps times (one more round warms up); best and median per leg.  One JSON line on stdout, and --out FILE.
    python tools/restore_probe.py [--config sr3_16_128 --config ddpm_128] [--calls 200] [--replays 30] [--reps 5] [--out FILE]   (GPU box)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def timed(fn, n, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def summary(ms):
    return {'best': min(ms), 'median': statistics.median(ms)}


def tails(shape, dev, a, torch, L, X):
    lib = L.load()
    B, Cc, H, W = shape
    n = B * Cc * H * W
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    x, eps, z, known = (torch.randn(shape, device=dev) for _ in range(4))
    mask1 = (torch.rand((B, 1, H, W), device=dev) < 0.5).float()
    maskc = (torch.rand(shape, device=dev) < 0.5).float()
    gray = torch.rand((B, 1, H, W), device=dev) * 2 - 1
    ymean = torch.rand((B, Cc, H // 8, W // 8), device=dev) * 2 - 1
    tabs = [torch.full((4,), v, device=dev) for v in (0.9, 0.43, 0.55, 0.45, 0.5)]
    tp = [L.ptr(t) for t in tabs]
    step2 = torch.zeros(2, dtype=torch.int32, device=dev)
    wa, wp = (X._floats(w) for w in X.gray_weights('rec601', Cc))
    ra, rs = torch.tensor([0.8, 1.0, 1.0, 1.0], device=dev), torch.tensor([0.6, 0.0, 0.0, 0.0], device=dev)
    to = torch.tensor([2, 0, 1, 2], dtype=torch.int32, device=dev)

    def restore(op, target, mask, mc):
        def f():
            step2.fill_(2)
            L.check(lib.sr3_restore_step(L.ptr(x), L.ptr(eps), L.ptr(z), op, L.ptr(target), L.ptr(mask), mc, wa, wp, B, Cc, H, W, 1.0, *tp,
                                         L.ptr(step2), 1, None, None, stream()))
        return f

    def consistent():
        step2.fill_(2)
        L.check(lib.sr3_consistent_step(L.ptr(x), L.ptr(eps), L.ptr(z), L.ptr(ymean), B, Cc, H, W, 8, 1.0, *tp, L.ptr(step2), 1, None, None,
                                        stream()))

    def jump():
        step2.fill_(-1)
        L.check(lib.sr3_travel_back_f32(L.ptr(x), L.ptr(z), L.ptr(ra), L.ptr(rs), L.ptr(to), 4, L.ptr(step2), B, Cc * H * W, stream()))

    def fill_only():                     # what every leg above pays for putting the counter back
        step2.fill_(2)
    plane = B * H * W
    legs = {      # name -> (call, fp32 values moved: x in and out, eps, z, the target and the mask)
        'fill_only': (fill_only, 0),
        'consistent_step_block8': (consistent, 4 * n + n // 64),
        'restore_mask_1plane': (restore(0, known, mask1, 1), 5 * n + plane),
        'restore_mask_cplanes': (restore(0, known, maskc, Cc), 6 * n),
        'restore_gray': (restore(1, gray, None, 0), 4 * n + plane),
        'travel_back': (jump, 3 * n),
    }
    ms = {k: [] for k in legs}
    for rep in range(a.reps + 1):
        for name, (fn, _) in legs.items():
            t = timed(fn, a.calls, torch)
            if rep:
                ms[name].append(t)
            x.copy_(known)               # (the in-place legs would otherwise drive x to infinity over thousands of calls)
    out = {}
    for name, (_, vals) in legs.items():
        s = summary(ms[name])
        us = (s['best'] - min(ms['fill_only'])) * 1e3 if name != 'fill_only' else s['best'] * 1e3
        out[name] = dict(us_best=s['best'] * 1e3, us_median=s['median'] * 1e3, bytes=4 * vals,
                         gb_per_s_net_of_fill=(4 * vals / (us * 1e-6) / 1e9) if vals and us > 0 else None)
    return out


def steps(name, cfg, netG, dev, a, torch, X):
    B, S = cfg['batch'], cfg['size']
    shape = (B, 3, S, S)
    cond = (torch.rand(shape, device=dev) * 2 - 1) if cfg['conditional'] else None
    N = a.replays
    legs = {'fused': {}, 'restore_mask': dict(restore=('mask',)), 'restore_gray': dict(restore=('gray', 1.0, 'rec601'))}
    if cond is not None:
        legs['consistency_block8'] = dict(consistency=8)
    states = {}
    netG.set_sampler(N, 0.0)
    for leg, spec in legs.items():
        netG.set_restore(None)
        netG.set_consistency(spec.get('consistency'))
        netG.set_restore(*spec.get('restore', (None,)))
        st = netG._loop_state(shape, shape if cond is not None else None, dev, consistency=netG.consistency, restore=netG.restore)
        netG.denoise_fn.ensure_derived()
        if cond is not None:
            st['cond'].copy_(cond)
        known = torch.rand(shape, device=dev) * 2 - 1
        if netG.consistency is not None:
            st['ymean'].copy_(X.block_means(known, 8))
        if netG.restore is not None:
            target = (known, (torch.rand((B, 1, S, S), device=dev) < 0.5).float()) if netG.restore['operator'] == 'mask' else known
            X.RESTORE.prepare(st, st['restore'], shape, target, dev)
        netG._capture(st)
        states[leg] = st
    netG.set_consistency(None)
    netG.set_restore(None)
    ms = {k: [] for k in legs}
    for rep in range(a.reps + 1):
        for leg, st in states.items():
            st['img'].copy_(torch.randn(shape, device=dev))
            st['step'].fill_(N - 1)
            t = timed(st['graph'].replay, N, torch)
            assert int(st['step'][1].item()) == -1 and bool(torch.isfinite(st['img']).all())
            if rep:
                ms[leg].append(t)
    return {leg: dict(ms_best=min(v), ms_median=statistics.median(v)) for leg, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', action='append', default=[])
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--replays', type=int, default=30)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import model.networks as networks
    from sr3_hip import lib as L
    from sr3_hip import x0_rules as X
    if not torch.cuda.is_available():
        sys.exit('restore_probe measures on the GPU; there is none here')
    dev = torch.device('cuda', 0)
    rec = {'what': 'restore step', 'calls': a.calls, 'replays': a.replays, 'reps': a.reps, 'configs': {}}
    for name in (a.config or ['sr3_16_128', 'ddpm_128']):
        cfg = bench.CONFIGS[name]
        torch.manual_seed(0)
        opt = bench.config_opt(name, n_timestep=2000)
        netG = networks.define_G(opt).to(dev)
        netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
        netG.eval()
        netG.show_progress = False
        netG.max_cached_loops = 4
        shape = (cfg['batch'], 3, cfg['size'], cfg['size'])
        rec['configs'][name] = dict(shape=list(shape), tails=tails(shape, dev, a, torch, L, X), steps=steps(name, cfg, netG, dev, a, torch, X))
        del netG
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(rec, indent=1, sort_keys=True) + '\n')


if __name__ == '__main__':
    main()
