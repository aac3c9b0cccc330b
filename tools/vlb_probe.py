#!/usr/bin/env python3
"""What the per-image terms of the variational bound cost, two measurements on one box:

(a) the training step of the benchmarked shape (bench.py's sr3_16_128: SR3 16 -> 128, batch 64, dropout 0.2) through
    EngineUNet.train_step on fixed inputs: the plain step (sr3_train_step_ex) against the step that also returns the per-image terms
    (sr3_train_step_ex3, one more launch pair over about 5C planes), and -- with --parent-pkg, the package directory of a build of the
    parent commit -- the parent's plain step.  Every leg runs in a child process of its own; the legs alternate --reps times.
(b) one replayed step of calc_bpd_loop against one replayed reverse step of the same net (bench.py's sampling shape, batch 16, a
    100-step schedule): the forward plus q_sample at the counter and the two launches of the terms, against the fused step.

One JSON line.    python tools/vlb_probe.py [--parent-pkg DIR] [--steps 30] [--reps 3] [--replays 100]   (GPU box)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def _opt(phase, n_timestep):
    sys.path.insert(0, ROOT)
    import bench
    return bench.config_opt('sr3_16_128', n_timestep=n_timestep, phase=phase), bench.CONFIGS['sr3_16_128']


def train_child(leg, steps, warmup):
    """ms per training step (forward + backward, no optimizer) of one leg: 'plain' or 'terms'."""
    import numpy as np
    import torch
    import model as Model
    opt, c = _opt('train', 2000)
    torch.manual_seed(1000)
    np.random.seed(1234)
    m = Model.create_model(opt)
    netG, un = m.netG, m.netG.denoise_fn
    dev = m.device
    B, S = c['train_batch'], c['size']
    g = torch.Generator().manual_seed(77)
    hr, sr = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev), (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    z = torch.randn(B, 3, S, S, generator=g).to(dev)
    t = np.arange(B) * (netG.num_timesteps // B)
    gam = torch.FloatTensor(netG.sqrt_alphas_cumprod_prev[t + 1]).to(dev)
    ca, cb = gam, (1 - gam ** 2).sqrt()
    kw = dict(grad_scale=1.0 / hr.numel())
    if leg == 'terms':
        from sr3_hip import diffusion as D
        tabs = D.ancestral_tables(netG._alphas_cumprod64, netG.num_timesteps)
        kw['per_image'] = torch.tensor(D.hybrid_step_scalars(tabs, t), dtype=torch.float32).to(dev)
    for _ in range(warmup):
        un.train_step(hr, sr, z, ca, cb, gam, None, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        un.train_step(hr, sr, z, ca, cb, gam, None, **kw)
    torch.cuda.synchronize()
    print(json.dumps({'ms': (time.perf_counter() - t0) / steps * 1e3}))


def eval_child(replays):
    import torch
    import model as Model
    opt, c = _opt('val', 100)
    torch.manual_seed(1000)
    m = Model.create_model(opt)
    netG = m.netG
    netG.show_progress = False
    dev = m.device
    B, S = c['batch'], c['size']
    g = torch.Generator().manual_seed(78)
    hr, sr = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev), (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    netG.calc_bpd_loop({'HR': hr, 'SR': sr})
    netG.super_resolution(sr)
    graphs = {'bpd_step': next(v for k, v in netG._loop_cache.items() if k[0] == 'bpd'),
              'reverse_step': next(v for k, v in netG._loop_cache.items() if k[0] != 'bpd')}
    rec = {k: [] for k in graphs}
    for _ in range(3):
        for k, st in graphs.items():
            st['step'].fill_(99)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replays):
                st['graph'].replay()
            torch.cuda.synchronize()
            rec[k].append((time.perf_counter() - t0) / replays * 1e3)
    print(json.dumps({k: {'best_ms': min(v), 'median_ms': statistics.median(v)} for k, v in rec.items()}))


def child(pkg, *args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=env, check=True, stdout=subprocess.PIPE,
                         timeout=300).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-pkg', default=None)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--replays', type=int, default=100)
    ap.add_argument('--child', nargs='*', default=None)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == 'train':
            train_child(args.child[1], int(args.child[2]), int(args.child[3]))
        else:
            eval_child(int(args.child[1]))
        return
    legs = [('plain', PKG), ('terms', PKG)] + ([('parent_plain', args.parent_pkg)] if args.parent_pkg else [])
    ms = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, pkg in legs:
            ms[name].append(child(pkg, '--child', 'train', 'terms' if name == 'terms' else 'plain', args.steps, args.warmup)['ms'])
    rec = {'train_step_ms': {k: {'best': min(v), 'median': statistics.median(v), 'all': v} for k, v in ms.items()},
           'eval_step': child(PKG, '--child', 'eval', args.replays), 'steps': args.steps, 'reps': args.reps}
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
