#!/usr/bin/env python3
"""What scale-shift time conditioning (config key model.unet.scale_shift_norm) costs next to the additive form, GPU only,
on random weights.  Device-event times after a warm-up, the two networks ALTERNATED in one process (round-robin, best of `--rounds`):

  (1) the reverse step of the flagship SR3 16 -> 128 network at batch 16 (graph replay), key absent against true;
  (2) the training step at batch 64 (dropout as configured, optimize_parameters), likewise.

    python tools/scale_shift_probe.py [--rounds 5] [--out profiles/scale_shift_probe.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30, help='graph replays per timing of the reverse step')
    ap.add_argument('--train-steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scale_shift_probe.json'))
    a = ap.parse_args()
    for p in (os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), ROOT, PKG):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import bench
    import model as Model
    import model.networks as networks
    from attn_heads_probe import alternate
    from wino_ragged_probe import step_ms
    d = torch.device('cuda', 0)
    rec = {'what': 'tools/scale_shift_probe.py: device-event times, the two networks alternated in one process, best of %d rounds; random weights'
                   % a.rounds, 'device': torch.cuda.get_device_name(0)}
    forms = {'absent': None, 'scale_shift_norm': True}

    nets = {}
    for key, flag in forms.items():
        torch.manual_seed(0)
        opt = bench.config_opt('sr3_16_128')
        if flag:
            opt['model']['unet']['scale_shift_norm'] = True
        n = networks.define_G(opt).to(d)
        n.set_new_noise_schedule(opt['model']['beta_schedule']['val'], d)
        n.show_progress = False
        nets[key] = n
    best = {k: 1e30 for k in nets}
    for _ in range(a.rounds):
        for k, n in nets.items():
            best[k] = min(best[k], step_ms(n, 128, 128, 16, a.steps))
    rec['reverse_step_ms_batch16'] = dict({k: round(v, 4) for k, v in best.items()},
                                          scale_shift_over_absent=round(best['scale_shift_norm'] / best['absent'], 4),
                                          launches={k: n.denoise_fn.plan.num_ops(16) for k, n in nets.items()},
                                          modulated_folds=sum(1 for _, row in nets['scale_shift_norm'].denoise_fn.plan.fold_list(16) if row >= 0))
    print('reverse step', rec['reverse_step_ms_batch16'], flush=True)
    del nets

    models = {}
    S, Bt = 128, 64
    g = torch.Generator().manual_seed(77)
    data = {'HR': torch.rand(Bt, 3, S, S, generator=g) * 2 - 1, 'SR': torch.rand(Bt, 3, S, S, generator=g) * 2 - 1}
    for key, flag in forms.items():
        torch.manual_seed(1000)
        np.random.seed(1234)
        opt = bench.config_opt('sr3_16_128', phase='train')
        if flag:
            opt['model']['unet']['scale_shift_norm'] = True
        m = Model.create_model(opt)
        m.feed_data(data)
        models[key] = m
    t = alternate(torch, {k: m.optimize_parameters for k, m in models.items()}, a.train_steps, a.rounds)
    rec['train_step_ms_batch64'] = dict({k: round(v / 1e3, 3) for k, v in t.items()},
                                        scale_shift_over_absent=round(t['scale_shift_norm'] / t['absent'], 4))
    print('train step', rec['train_step_ms_batch64'], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
