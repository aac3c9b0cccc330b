#!/usr/bin/env python3
"""Bits per dimension of a checkpoint over the validation set, split by timestep (improved-diffusion's image_nll.py on this engine):
every item of the config's datasets.val goes through DDPM.calc_bpd (EngineDiffusion.calc_bpd_loop) on the val phase's schedule -- the
weights of path.resume_state, the EMA weights where train.ema_scheduler.enabled is set -- and the per-image totals, prior terms and
per-step terms are averaged over the images.  Image k draws its noise from the validation stream of item k (sr3_hip.dist.val_item_seed),
so the numbers do not depend on --batch; the streams' base is SR3_VAL_SEED, else --seed (default 0): the same command gives the same
numbers.  One JSON line:

    {"metric": "bpd", "value": mean total, "prior_bpd": ..., "vb": [per step, j = 0 .. S - 1], "x0_mse": [...], "steps": S, "images": N}

    python tools/image_nll.py -c config/sr_sr3_16_128.json [--steps S] [--max-images N] [--batch 8] [--seed 0]   (GPU box)
--steps: the respaced walk's length (default: all T steps of the val schedule): what an S-step ancestral sampler gives up in likelihood."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')
sys.path.insert(0, PKG)


def load_config(path):
    """The reference's config format: JSON with // comments (core/logger.py: parse); phase val on GPU 0."""
    with open(path) as f:
        text = '\n'.join(re.sub(r'//.*$', '', line) if not re.search(r'"[^"]*//[^"]*"', line) else line for line in f.read().splitlines())
    opt = json.loads(text)
    opt['phase'] = 'val'
    opt['gpu_ids'] = [0]
    opt.setdefault('distributed', False)
    opt.setdefault('path', {}).setdefault('resume_state', None)
    opt['model'].setdefault('finetune_norm', False)
    return opt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-c', '--config', required=True)
    ap.add_argument('--steps', type=int, default=None)
    ap.add_argument('--max-images', type=int, default=None)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    import torch
    import torch.utils.data
    import data as Data
    import model as Model
    from sr3_hip import dist as _dist
    torch.manual_seed(args.seed)         # (the base of the validation items' noise streams, sr3_hip.dist.val_base_seed, unless SR3_VAL_SEED is set)
    opt = load_config(args.config)
    dopt = opt['datasets']['val']
    dataset = Data.create_dataset(dopt, 'val')
    m = Model.create_model(opt)
    m.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    m.netG.show_progress = False
    loader = Data.DeviceBatches(torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=0), m.device)
    sums, n, first = None, 0, 0
    group = []

    def flush():
        nonlocal sums, n, first
        batch = {k: torch.cat([b[k] for b in group], 0) for k in ('HR', 'SR') if k in group[0]}
        m.netG.eval()
        with torch.no_grad(), m._sampling_weights():
            x_in = batch if m.netG.conditional else batch['HR']
            out = m.netG.calc_bpd_loop(x_in, steps=args.steps, item_seeds=[_dist.val_item_seed(first + k, 0) for k in range(len(group))])
        part = {k: v.double().sum(0) for k, v in out.items()}
        sums = part if sums is None else {k: sums[k] + part[k] for k in part}
        n += len(group)
        first += len(group)
        del group[:]
    for item in loader:
        if args.max_images is not None and first + len(group) >= args.max_images:
            break
        if group and item['HR'].shape != group[0]['HR'].shape:
            flush()
        group.append(item)
        if len(group) == args.batch:
            flush()
    if group:
        flush()
    if not n:
        raise SystemExit('image_nll: the validation set is empty')
    mean = {k: (v / n).cpu() for k, v in sums.items()}
    print(json.dumps({'metric': 'bpd', 'value': float(mean['total_bpd']), 'prior_bpd': float(mean['prior_bpd']),
                      'vb': [float(v) for v in mean['vb']], 'x0_mse': [float(v) for v in mean['x0_mse']],
                      'steps': int(mean['vb'].numel()), 'images': n, 'config': os.path.basename(args.config)}))


if __name__ == '__main__':
    main()
