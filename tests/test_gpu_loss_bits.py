"""The loss kernels' bits (sr3_loss_grad_f32, sr3_hybrid_loss_grad_f32): equality with a recording, not closeness.

tests/golden/loss_grad_bits.json holds, per case, the loss -- and the hybrid op's vlb sum -- as float bits and the sha256 of g's bytes,
recorded on an MI355X from the library as it was while train_kernels.hip wrote the L1 / L2 / Huber lane, the block reduction and the
k_sum_parts tail out in each of k_l1_loss_grad, k_loss_grad and k_hybrid_loss_grad.  Whatever states them once has to keep:
  - the plain path (NULL tables, L1 / L2 through sr3_loss_grad_f32) adding each channel's rho straight into the thread's double sum,
    the other paths summing a pixel's channels first: the two groupings round differently;
  - d = z - e on the plain path, (az z + (tb ? ax hr : 0)) - e on the others: with NULL tables they differ in the sign of a zero
    (-0.f + 0.f is +0.f), which for L2 reaches g;
  - the hybrid kernel's two reductions and loss_part's [blocks | blocks] layout.
The inputs carry z == e exactly, -0.0 in z against +0.0 in e, |d| below, at and above the Huber delta, hr beyond +-0.999 and rows with
the last-step flag set and clear.  Shapes: 35 pixels an image (a block's tail, the pad lanes, one channel and three), and 3 x 22500 =
67500 pixels over the grid's 65536 threads (the grid-stride loop's second, ragged trip).

Record again (on the GPU, only from a library whose bits are the wanted ones):  SR3_LIBRARY=/path/lib.so python tests/test_gpu_loss_bits.py [out.json]
"""
import ctypes as C
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch                                                     # (before the library: it binds to the HIP runtime torch loaded)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loss_grad_bits.json')
SHAPES = [(2, 3, 35), (2, 1, 35), (3, 3, 22500)]      # (B, C, HW)
DELTA = 1.0
SCALE = 2.0 ** -10
LAMBDA = 0.001
TA, TB, W = (1.0, 0.5, 0.9), (0.0, -0.85, -0.4), (1.0, 1.5, 0.375)      # per image; image 0: target z exactly, so the planted d survive the tables
CASES = [(s, entry, tables, kind) for s in SHAPES for entry in ('loss', 'hybrid') for tables in (False, True) for kind in (0, 1, 2)]

_inputs = {}


def case_id(c):
    (B, Cc, HW), entry, tables, kind = c
    return '%dx%dx%d-%s-%s-kind%d' % (B, Cc, HW, entry, 'tables' if tables else 'plain', kind)


def inputs(shape):
    """the host inputs of one shape, built once: fp32 arrays from a seeded NumPy generator with the special elements planted"""
    if shape in _inputs:
        return _inputs[shape]
    B, Cc, HW = shape
    rng = np.random.default_rng(20240 + 7 * HW + Cc)
    f32 = np.float32
    z = rng.standard_normal((B, Cc, HW)).astype(f32)
    e = (0.8 * rng.standard_normal((B, Cc, HW))).astype(f32)
    v = rng.uniform(-1.0, 1.0, (B, Cc, HW)).astype(f32)                  # the raw variance head
    hr = rng.uniform(-1.0, 1.0, (B, Cc, HW)).astype(f32)
    xt = rng.standard_normal((B, Cc, HW)).astype(f32)
    for b in range(B):                      # in every image (image 0 keeps them under the tables: ta 1, tb 0), channel 0
        e[b, 0, 0] = z[b, 0, 0]                                          # z == e
        z[b, 0, 1], e[b, 0, 1] = f32(-0.0), f32(0.0)                     # d = -0 on the plain path, +0 behind the tables' sum
        z[b, 0, 2], e[b, 0, 2] = f32(0.0), f32(0.0)
        z[b, 0, 3], e[b, 0, 3] = f32(1.5), f32(0.5)                      # |d| == delta
        z[b, 0, 4], e[b, 0, 4] = f32(1.5), f32(0.5 - 2.0 ** -23)         # one ulp above
        z[b, 0, 5], e[b, 0, 5] = f32(1.5), f32(0.5 + 2.0 ** -24)         # one ulp below
        z[b, 0, 6], e[b, 0, 6] = f32(-1.5), f32(-0.5)                    # d == -delta
        z[b, 0, 7], e[b, 0, 7] = f32(0.25), f32(3.0)                     # far outside
        hr[b, 0, 8:14] = np.array([-1.0, -0.9995, -0.999, 0.999, 0.9995, 1.0], dtype=f32)      # the open bins of the last step and their edges
    assert np.signbit(z[0, 0, 1]) and not np.signbit(e[0, 0, 1])
    d = z[0].astype(np.float64) - e[0]
    assert (np.abs(d) == DELTA).sum() >= 2 and (np.abs(d) < DELTA).any() and (np.abs(d) > DELTA).any() and (d == 0).sum() >= 3
    assert (np.abs(hr) > 0.999).sum() >= 4 * B
    # step_scalars [B, 8]: a, b, c1, c2, log beta, log beta~, last, 0 -- image 0 on the walk's last step, the others inside it
    scal = np.zeros((B, 8), dtype=f32)
    for b in range(B):
        scal[b, :7] = [1.005, 0.1, 1.0, 0.0, np.log(1e-4), np.log(2e-5), 1.0] if b == 0 else \
                      [1.25 + 0.5 * b, 0.75 + 0.8 * b, 0.2 / b, 0.8, np.log(0.02 * b), np.log(0.012 * b), 0.0]
    out2 = np.concatenate([e, v], axis=1)                                # [B, 2 Cc, HW]: the prediction, then the variance head
    tabs = tuple(np.array(t[:B], dtype=f32) for t in (TA, TB, W))
    _inputs[shape] = dict(z=z, e=e, out2=out2, hr=hr, xt=xt, scal=scal, tabs=tabs)
    return _inputs[shape]


def run(lib, c):
    """-> {'loss': float bits, 'vlb': float bits (hybrid), 'g': sha256 of g's bytes} of one case on the device"""
    import gpu_util as G
    from sr3_hip import lib as L
    (B, Cc, HW), entry, tables, kind = c
    h = inputs((B, Cc, HW))
    d = G.dev()
    t = {k: torch.from_numpy(h[k]).to(d) for k in ('z', 'e', 'out2', 'hr', 'xt', 'scal')}
    tz, tx, w = (torch.from_numpy(a).to(d) for a in h['tabs']) if tables else (None, None, None)
    loss = torch.full((1,), float('nan'), device=d)
    vlb = torch.full((1,), float('nan'), device=d)
    if entry == 'loss':
        g = torch.full((B, HW, 4), float('nan'), device=d)
        scratch = torch.empty(int(lib.sr3_loss_grad_scratch_bytes()), dtype=torch.uint8, device=d)
        L.check(lib.sr3_loss_grad_f32(L.ptr(t['z']), L.ptr(t['e']), L.ptr(t['hr']), L.ptr(tz), L.ptr(tx), L.ptr(w), B, Cc, HW, kind,
                                      C.c_float(DELTA), C.c_float(SCALE), L.ptr(g), L.ptr(loss), L.ptr(scratch), G.stream()))
    else:
        g = torch.full((B, HW, 8), float('nan'), device=d)
        scratch = torch.empty(int(lib.sr3_hybrid_loss_grad_scratch_bytes()), dtype=torch.uint8, device=d)
        L.check(lib.sr3_hybrid_loss_grad_f32(L.ptr(t['z']), L.ptr(t['out2']), L.ptr(t['hr']), L.ptr(t['xt']), L.ptr(tz), L.ptr(tx), L.ptr(w),
                                             L.ptr(t['scal']), C.c_float(LAMBDA), B, Cc, HW, kind, C.c_float(DELTA), C.c_float(SCALE),
                                             L.ptr(g), L.ptr(loss), L.ptr(vlb), L.ptr(scratch), G.stream()))
    torch.cuda.synchronize()
    bits = lambda x: struct.unpack('<I', struct.pack('<f', float(x)))[0]
    gh = g.cpu().numpy()
    assert np.isfinite(gh).all(), 'an element of g was not written'
    got = {'loss': bits(loss), 'g': hashlib.sha256(gh.tobytes()).hexdigest()}
    if entry == 'hybrid':
        got['vlb'] = bits(vlb)
    return got


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)
    assert all(len(v['g']) == 64 and ('vlb' in v) == ('hybrid' in k) for k, v in recorded.items())


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_loss_bits_are_the_recorded_ones(recorded, c):
    from sr3_hip import lib as L
    got = run(L.load(), c)
    want = recorded[case_id(c)]
    print('%s: got %s, recorded %s' % (case_id(c), got, want))
    assert got == want


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    sys.path[:0] = [root, os.path.join(root, 'image-super-resolution-via-iterative-refinement_amd'), here]
    from sr3_hip import lib as L
    lib = L.load()
    out = {case_id(c): run(lib, c) for c in CASES}
    again = {case_id(c): run(lib, c) for c in CASES}
    assert out == again, 'two runs of the same library differ: nothing to pin'
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d cases from %s into %s' % (len(out), L.LIB_PATH, path))
