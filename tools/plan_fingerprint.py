#!/usr/bin/env python3
"""Host-side fingerprint of everything the planner decides (no GPU needed): the launch list of every network under every plan
option, batch size and geometry, the per-op scratch / statistics-slice queries over a grid of shapes and ABI tile numbers, and
the training workspace size (or refusal) of every network under train_geom at every geometry and option.

  python tools/plan_fingerprint.py --out full.jsonl          one JSON record per case (what to diff between two builds)
  python tools/plan_fingerprint.py --golden COMMIT           rewrite tests/golden/plan_fingerprint.json: per-case SHA-256 + size

Two builds of the library choose the same kernels exactly when their outputs are byte-identical.  A/B: build the other library
into a scratch directory (SR3_BUILD_DIR / SR3_OUT of csrc/build.sh) and load it with SR3_LIBRARY.
tests/test_plan_fingerprint_cpu.py holds the built library to the committed digests; a planner change regenerates them on purpose
(--golden), and the diff of the fixture then names the cases that moved."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'image-super-resolution-via-iterative-refinement_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from sr3_hip import engine as E, lib as L      # noqa: E402
from dump_plan import CONFIGS                   # noqa: E402
from helpers import DESCS                       # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'plan_fingerprint.json')
BATCHES = (1, 2, 3, 4, 16, 32, 64)
GEOMETRIES = {'sr3_16_128': ((128, 192), (176, 128), (256, 256), (64, 64))}       # (height, width) beside the native one
OPTIONS = ([('default', None)]
           + [(k, 0) for k in ('fuse_stats', 'fuse_res', 'winograd', 'wino_split', 'wino_split8', 'wino2', 'wino_ragged', 'gemm_split')]
           + [('gemm_wpre', 1)] + [(k, 0) for k in ('gemm2', 'gemm_s2', 'gemm_n64', 'fold_fuse')]
           + [('fork_side', 1), ('attn_long', 1), ('keep_all', 1)]
           + [('gemm_tile', v) for v in (1, 2, 3, 4)] + [('tile_cfg', v) for v in (1, 2, 3, 4, 5, 6, 9, 11)]
           + [('ksplit', v) for v in (1, 2, 4)])
# training plans (train_geom = 1): every network x batch x geometry under each of these, appended behind the cases above
TRAIN_BATCHES = (1, 2, 4, 16, 64)
TRAIN_TINY_GEOMETRIES = ((16, 24), (24, 16), (80, 64))       # the networks of tests/helpers.py, beside their native 16 x 16
TRAIN_OPTIONS = ([('default', None)]
                 + [(k, 0) for k in ('winograd', 'wino_split', 'wino2', 'wino_ragged', 'gemm_split', 'gemm2', 'gemm_n64', 'fuse_res',
                                     'fuse_stats')]
                 + [('tile_cfg', 5), ('ksplit', 1)])
Q_BATCHES = (1, 4, 16)
Q_MAPS = ((4, 4), (8, 8), (11, 8), (16, 16), (22, 16), (32, 32), (64, 64), (128, 128))
Q_CHANNELS = (64, 128, 256, 320, 512, 1024)
Q_KSPLITS = (0, 1, 2, 4, 8)


def networks():
    for name in sorted(CONFIGS):
        yield name, CONFIGS[name]
    for name in sorted(DESCS):
        d = DESCS[name]
        yield name, (d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'],
                     d['attn_res'], d['res_blocks'], d['image_size'])


def last_error(lib):
    return (lib.sr3_last_error() or b'').decode()


def plan_case(args, geometry, option, value, batch):
    plan = E.Plan(*args)
    lib, h = plan.lib, plan.handle
    if option != 'default':
        plan.set_option(option, value)
    if geometry:
        plan.set_geometry(*geometry)
    rec = {}
    n = int(lib.sr3_plan_num_ops(h, batch))
    if n < 0:       # the plan is refused at this geometry: the return code and the whole text
        info = L.OpInfo()
        rec['refused'] = [int(lib.sr3_plan_op_info(h, batch, 0, C.byref(info))), last_error(lib)]
    else:
        side, wait = C.c_int(), C.c_int()
        ops = plan.op_list(batch)
        for i, o in enumerate(ops):
            L.check(lib.sr3_plan_op_side(h, batch, i, C.byref(side), C.byref(wait)))
            o['side_id'], o['wait_id'] = side.value, wait.value
            o['flops'] = repr(o['flops'])
        rec['ops'] = ops
    rec['workspace_bytes'] = int(lib.sr3_workspace_bytes(h, batch))
    rec['forward_flops'] = repr(float(lib.sr3_plan_forward_flops(h, batch)))
    rec['derived_bytes'] = int(lib.sr3_plan_derived_bytes(h))
    if option == 'keep_all':
        rec['taps'] = plan.taps()
    cond = plan.in_channel - plan.out_channel if plan.in_channel > plan.out_channel else 0
    rec['train_workspace_bytes'] = int(lib.sr3_train_workspace_bytes(h, batch, cond))
    if rec['train_workspace_bytes'] == 0:
        rec['train_refused'] = last_error(lib)
    return rec


def train_case(args, geometry, option, value, batch):
    """The training workspace size of one plan under train_geom, or the whole refusal text; a refused plan is asked again
    under attn_long."""
    plan = E.Plan(*args)
    lib, h = plan.lib, plan.handle
    plan.set_option('train_geom', 1)
    if option != 'default':
        plan.set_option(option, value)
    if geometry:
        plan.set_geometry(*geometry)
    cond = plan.in_channel - plan.out_channel if plan.in_channel > plan.out_channel else 0
    rec = {'train_workspace_bytes': int(lib.sr3_train_workspace_bytes(h, batch, cond))}
    if rec['train_workspace_bytes'] == 0:
        rec['train_refused'] = last_error(lib)
        plan.set_option('attn_long', 1)
        rec['attn_long_train_workspace_bytes'] = int(lib.sr3_train_workspace_bytes(h, batch, cond))
        if rec['attn_long_train_workspace_bytes'] == 0:
            rec['attn_long_train_refused'] = last_error(lib)
    return rec


def query_case(lib, B, H, W):
    scratch, slices = [], []
    for cin in Q_CHANNELS:
        for cout in Q_CHANNELS:
            for tile in range(25):
                for ks in Q_KSPLITS:
                    for ksize in (1, 3):
                        scratch.append(int(lib.sr3_conv_scratch_bytes(B, H, W, cin, cout, ksize, tile, ks)))
                    for ups in (0, 1):
                        slices.append(int(lib.sr3_conv_stats_slices(B, H, W, ups, cin, cout, tile, ks)))
    # order of both lists: Cin, Cout, tile_cfg 0..24, ksplit, then ksize 1, 3 (scratch) / ups 0, 1 (slices)
    return {'conv_scratch_bytes': scratch, 'conv_stats_slices': slices}


def cases():
    """(case id, record) in a fixed order."""
    for name, args in networks():
        for geometry in (None,) + GEOMETRIES.get(name, ()):
            for option, value in OPTIONS:
                for batch in BATCHES:
                    cid = 'plan/%s/%s/%s/B%d' % (name, '%dx%d' % geometry if geometry else 'native',
                                                 option if value is None else '%s=%d' % (option, value), batch)
                    yield cid, plan_case(args, geometry, option, value, batch)
    lib = L.load()
    for B in Q_BATCHES:
        for H, W in Q_MAPS:
            yield 'query/B%d/%dx%d' % (B, H, W), query_case(lib, B, H, W)
    for name, args in networks():
        for geometry in (None,) + GEOMETRIES.get(name, ()) + (TRAIN_TINY_GEOMETRIES if name in DESCS else ()):
            for option, value in TRAIN_OPTIONS:
                for batch in TRAIN_BATCHES:
                    cid = 'train/%s/%s/%s/B%d' % (name, '%dx%d' % geometry if geometry else 'native',
                                                  option if value is None else '%s=%d' % (option, value), batch)
                    yield cid, train_case(args, geometry, option, value, batch)


def dumps(rec):
    return json.dumps(rec, sort_keys=True, separators=(',', ':'))


def digest(rec):
    """[SHA-256 of the record, its size: ops of a plan, values of a query case, 0 for a refused plan]."""
    n = len(rec['ops']) if 'ops' in rec else len(rec.get('conv_scratch_bytes', ())) + len(rec.get('conv_stats_slices', ()))
    return [hashlib.sha256(dumps(rec).encode()).hexdigest(), n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='write one JSON record per case to this file')
    ap.add_argument('--golden', metavar='COMMIT', help='rewrite %s; COMMIT names the source the loaded library was built from'
                    % os.path.relpath(GOLDEN, ROOT))
    a = ap.parse_args()
    if not a.out and not a.golden:
        ap.error('nothing to do: --out and / or --golden')
    out = open(a.out, 'w') if a.out else None
    digests = {}
    for cid, rec in cases():
        digests[cid] = digest(rec)
        if out:
            out.write(dumps({'case': cid, 'record': rec}) + '\n')
    if out:
        out.close()
    if a.golden:
        with open(GOLDEN, 'w') as f:
            f.write('{"generated_from": %s,\n "cases": {\n' % json.dumps(a.golden))
            f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in digests.items()))
            f.write('\n }}\n')
    print('%d cases' % len(digests))


if __name__ == '__main__':
    main()
