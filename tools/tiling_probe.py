#!/usr/bin/env python3
"""What a tiled reverse step costs next to the whole-image step: the `sr3_16_128` network on one conditional image
of --sizes (512 and 1024 squared), the captured tiled step (128 x 128 tiles, --overlap, --tile-batch per forward) against the captured
whole-image step with `long_attention`, each replayed --replays times per repetition and timed with HIP events, legs interleaved; then
the share of the tiled step spent in the two kernels of csrc/tiled.hip: sr3_tile_gather over all tiles and sr3_tiled_step alone (no
forward, no draw), each captured into a graph of its own on the step's buffers and replayed the same way.  Both legs run under set_sampler(replays, 1.0): one table row per replay, z drawn every step.
    python tools/tiling_probe.py [--sizes 512 1024] [--tile 128] [--overlap 32] [--tile-batch 16] [--replays 20] [--reps 3]   (GPU box)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd')


def timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 1024])
    ap.add_argument('--tile', type=int, default=128)
    ap.add_argument('--overlap', type=int, default=32)
    ap.add_argument('--tile-batch', type=int, default=16)
    ap.add_argument('--replays', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-whole', action='store_true', help='skip the whole-image leg')
    a = ap.parse_args()
    sys.path.insert(0, PKG)
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import model.networks as networks
    dev = torch.device('cuda', 0)
    N = a.replays

    def build(long_attention):
        torch.manual_seed(0)
        opt = bench.config_opt('sr3_16_128', n_timestep=2000)
        opt['model']['unet']['long_attention'] = long_attention
        netG = networks.define_G(opt).to(dev)
        netG.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
        netG.eval()
        netG.show_progress = False
        netG.set_sampler(N, 1.0)
        return netG
    tiled_net = build(False)
    whole_net = None if a.no_whole else build(True)
    rec = {'what': 'tiled step', 'config': 'sr3_16_128', 'tile': a.tile, 'overlap': a.overlap, 'tile_batch': a.tile_batch,
           'replays': N, 'reps': a.reps, 'sizes': {}}
    for S in a.sizes:
        cond = torch.rand(1, 3, S, S, device=dev) * 2 - 1
        legs = {}
        tiled_net.p_sample_loop_tiled(cond, tile=a.tile, overlap=a.overlap, tile_batch=a.tile_batch)      # capture + one warm chain
        legs['tiled'] = next(reversed(tiled_net._loop_cache.values()))
        if whole_net is not None:
            whole_net.p_sample_loop(cond)
            legs['whole'] = next(reversed(whole_net._loop_cache.values()))
        ms = {k: [] for k in legs}
        for rep in range(a.reps):
            for name, st in legs.items():
                st['img'].normal_()
                st['step'].fill_(N - 1)
                ms[name].append(timed(st['graph'].replay, N))
                assert int(st['step'][1].item()) == -1 and bool(torch.isfinite(st['img']).all())
        st = legs['tiled']
        out = {'tiles': st['grid'].n_tiles, 'chunks': [n for _, n in st['chunks']]}
        for name in legs:
            out['ms_per_step_' + name] = {'best': min(ms[name]), 'median': statistics.median(ms[name])}
        # the two new kernels alone, on the step's own buffers, each leg captured into a small graph of its own so that the share is
        # device time over device time (an eager call would add one host launch per chunk to kernels that take microseconds)
        total = st['eps_tiles'].shape[0]

        def gather_all():
            for first, n in st['chunks']:
                tiled_net._gather_tiles(st, st['img'], st['x_tiles'][:n], first, n)

        def tail():                                      # the step without its forwards and without a draw: sr3_tiled_step alone
            tiled_net._one_step(st, draw_noise=False)
        g_gather, g_tail = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_gather):
            gather_all()
        chunks, st['chunks'] = st['chunks'], []
        with torch.cuda.graph(g_tail):
            tail()
        st['chunks'] = chunks
        t_gather = min(timed(g_gather.replay, N) for _ in range(a.reps))
        t_tail = []
        for _ in range(a.reps):
            st['step'].fill_(N - 1)                      # N replays walk the N table rows, as the step's graph does
            t_tail.append(timed(g_tail.replay, N))
            assert int(st['step'][1].item()) == -1
        t_tail = min(t_tail)
        out['ms_tile_gather_all_%d_tiles' % total] = t_gather
        out['ms_tiled_step'] = t_tail
        out['share_of_step_in_new_kernels'] = (t_gather + t_tail) / out['ms_per_step_tiled']['best']
        rec['sizes']['%dx%d' % (S, S)] = out
        tiled_net._loop_cache = {}
        if whole_net is not None:
            whole_net._loop_cache = {}
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
