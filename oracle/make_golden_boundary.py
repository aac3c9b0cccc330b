#!/usr/bin/env python3
"""tests/golden/ref_boundary.json: what tests/test_boundary_cpu.py compares the drop-in against, recorded from a reference tree
so that the tests stand without one:
  signatures    -- tests/sig_dump.py run on the reference's `model` package (names, parameter kinds, default reprs);
  init_weights  -- sha256 / shape / dtype of every `denoise_fn.*` tensor after the reference's init_weights(netG, init_type)
                   on the sr3_tiny network (seed 5 for define_G, seed 9 for the scheme);
  configs       -- the `model` subtree and train.optimizer.lr of the reference JSON configs bench.py restates.
    python oracle/make_golden_boundary.py <reference root>        (default: $SR3_REFERENCE)"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST = os.path.join(ROOT, 'tests', 'golden', 'ref_boundary.json')
INIT_TYPES = ('normal', 'kaiming', 'orthogonal')
REF_JSONS = {'sr3_16_128': 'config/sr_sr3_16_128.json', 'sr3_64_512': 'config/sr_sr3_64_512.json',
             'ddpm_128': 'config/sample_ddpm_128.json'}

# run in a fresh interpreter per tree (both call their package `model`); prints {name: [sha256, shape, dtype]}
INIT_CODE = '''
import hashlib, json, logging, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
logging.disable(50)
import torch
import model.networks as N
from helpers import opt_for
torch.manual_seed(5)
net = N.define_G(opt_for("sr3_tiny", phase="val", gpu=False))
torch.manual_seed(9)
N.init_weights(net, init_type=sys.argv[3], scale=0.3, std=0.05)
out = {k: [hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest(), list(v.shape), str(v.dtype)]
       for k, v in net.state_dict().items() if k.startswith("denoise_fn.")}
print(json.dumps(out, sort_keys=True))
'''


def init_digests(root, init_type):
    r = subprocess.run([sys.executable, '-c', INIT_CODE, root, os.path.join(ROOT, 'tests'), init_type], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, cwd=tempfile.gettempdir())
    if r.returncode != 0:
        raise RuntimeError(r.stderr.decode()[-800:])
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def signatures(root):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'sig_dump.py'), root], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.decode()[-800:])
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def config_subtrees(root):
    """The reference's JSON files with their // comments stripped as its core/logger.py:21-33 does."""
    out = {}
    for name, rel in REF_JSONS.items():
        with open(os.path.join(root, rel)) as f:
            full = json.loads('\n'.join(line.split('//')[0] for line in f))
        out[name] = {'ref_json': rel, 'model': full['model'], 'lr': full['train']['optimizer']['lr']}
    return out


def record(root):
    return {'signatures': signatures(root), 'init_weights': {t: init_digests(root, t) for t in INIT_TYPES},
            'configs': config_subtrees(root)}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('SR3_REFERENCE')
    if not root or not os.path.isfile(os.path.join(root, 'model', 'networks.py')):
        sys.exit('usage: make_golden_boundary.py <reference root> (or set SR3_REFERENCE)')
    with open(DST, 'w') as f:
        json.dump(record(root), f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', DST, os.path.getsize(DST), 'bytes')


if __name__ == '__main__':
    main()
