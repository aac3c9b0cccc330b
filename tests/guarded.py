"""Guarded device buffers for the scratch / workspace contract tests (a plain helper module).

`Guarded(nbytes, fill, dev, band)` is ONE uint8 allocation laid out as [front band | payload | back band]: the payload starts
256-byte aligned, the bands are multiples of 256 bytes, and every byte of all three holds `fill`.  A kernel that writes one byte
outside the payload changes a band (`intact()`), a kernel that reads outside it reads the fill (NaN for tensors), and a kernel that
reads its scratch before writing it sees whatever `fill` says the memory held before:

  Z  0x00  zeros: what a fresh allocation usually is (the baseline)
  N  0xFF  every fp32 / fp64 word a NaN, every int32 -1: reads that propagate
  F  0x4B  every fp32 ~ 1.3e7, every fp64 ~ 1e55, every int32 ~ 1.3e9, all finite: reads that a NaN-dropping op (fmaxf, clamps,
           selects) or a counter would hide from N

Bands are 1 MiB for workspaces and scratch, 16 KiB (the 4096 floats of the older guarded tests) for tensors.

`run_row` is the loop both per-op tables run their rows through: tests/scratch_rows.py (the scratch under Z, N and F, the operands' bands
NaN) and tests/edge_rows.py (every operand's bands under N and under F)."""
import ctypes as C

import torch

Z, N, F = 0x00, 0xFF, 0x4B
FILLS = (('Z', Z), ('N', N), ('F', F))
WS_BAND = 1 << 20
TENSOR_BAND = 4096 * 4


class Guarded(object):
    def __init__(self, nbytes, fill, dev, band=WS_BAND):
        assert band > 0 and band % 256 == 0 and nbytes >= 0
        self.nbytes, self.fill_byte, self.band = int(nbytes), int(fill), int(band)
        self.padded = (self.nbytes + 255) // 256 * 256          # the back band proper starts on the next 256-byte boundary
        self.raw = torch.empty(self.band + self.padded + self.band + 256, dtype=torch.uint8, device=dev)
        self.off = (-self.raw.data_ptr()) % 256 + self.band     # the payload's offset: 256-byte aligned, a whole band in front
        self.raw.fill_(self.fill_byte)

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + self.off)

    def fill(self, byte):
        """Refill the whole allocation, bands included, with another byte."""
        self.fill_byte = int(byte)
        self.raw.fill_(self.fill_byte)
        return self

    def view(self, dtype=torch.uint8, shape=None):
        item = torch.empty((), dtype=dtype).element_size()
        assert self.nbytes % item == 0
        v = self.raw[self.off:self.off + self.nbytes].view(dtype)
        return v if shape is None else v.view(*shape)

    def intact(self):
        """True when every byte outside the payload (the bands, and the alignment slack next to them) still holds the fill."""
        front, back = self.raw[:self.off], self.raw[self.off + self.nbytes:]
        return bool((front == self.fill_byte).all()) and bool((back == self.fill_byte).all())


def _item(dtype):
    return torch.empty((), dtype=dtype).element_size()


def tensor_in(t, dev, band=TENSOR_BAND, fill=N):
    """A guarded device copy of the CPU tensor `t` (contiguous) with NaN bands: a read outside it shows up in a result.  `fill`: another
    byte for the bands (F: a read that a NaN-dropping op would hide).  Returns (Guarded, device view)."""
    t = t.contiguous()
    g = Guarded(t.numel() * _item(t.dtype), fill, dev, band)
    v = g.view(t.dtype, tuple(t.shape))
    v.copy_(t)
    return g, v


def tensor_out(shape, dev, dtype=torch.float32, band=TENSOR_BAND, fill=N):
    """A guarded, NaN-filled output tensor: an element the call leaves unwritten shows up.  `fill`: another byte for the bands (the
    payload stays NaN).  Returns (Guarded, device view)."""
    n = 1
    for s in shape:
        n *= int(s)
    g = Guarded(n * _item(dtype), fill, dev, band)
    v = g.view(dtype, tuple(shape))
    if fill != N:
        g.raw[g.off:g.off + g.nbytes] = N
    return g, v


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


DUMMY_SCRATCH = 256


def run_row(row, lib, dev, stream, fills=FILLS, operands=False):
    """One row of a contract table (tests/scratch_rows.py, tests/edge_rows.py) under each of `fills`: the scratch is exactly the queried
    size between 1 MiB bands of the fill, every input sits between 16 KiB bands and every output is NaN-filled between such bands.
    Asserted per fill: rc 0, every band intact, every input bit-unchanged, every floating output finite; then the outputs bit-equal
    across the fills (a row may name, under `same`, its own comparison for an output that atomics accumulate).

    operands False (the scratch contract): the operands' bands are NaN under every fill, the row must have something in scratch, and
    the row's float64 check runs once.  operands True (the operand contract): the fill is that of every operand's bands too, a row
    whose query returns 0 gets a 256-byte dummy scratch that must come back untouched, and the check runs under every fill."""
    spec = row.spec()
    nb = spec['query'](lib)
    if not operands:
        assert nb > 0, 'the row has nothing in scratch'
    if spec.get('expect') is not None:
        assert nb == spec['expect'], (nb, spec['expect'])
    shared = None if operands else {k: tensor_in(v, dev)[0] for k, v in spec['ins'].items()}
    same = spec.get('same', {})
    results = []
    for name, byte in fills:
        ob = byte if operands else N
        ins = shared if shared is not None else {k: tensor_in(v, dev, fill=ob)[0] for k, v in spec['ins'].items()}
        scratch = Guarded(nb if nb > 0 else DUMMY_SCRATCH, byte, dev)
        guards = dict(ins, scratch=scratch)
        outs = {}
        for k, o in spec['outs'].items():
            if torch.is_tensor(o):          # in / out: starts from the row's value
                guards[k], outs[k] = tensor_out(tuple(o.shape), dev, dtype=o.dtype, fill=ob)
                outs[k].copy_(o)
            else:
                guards[k], outs[k] = tensor_out(o[0], dev, dtype=o[1], fill=ob)
        if spec.get('derived'):
            guards['derived'] = Guarded(spec['derived'], byte, dev)
        P = {k: g.ptr for k, g in guards.items() if k != 'scratch'}
        rc = spec['call'](lib, P, scratch.ptr, nb if nb > 0 else DUMMY_SCRATCH, stream)
        assert rc == 0, lib.sr3_last_error()
        torch.cuda.synchronize()
        for k, g in guards.items():
            assert g.intact(), '%s: a kernel wrote outside `%s` (fill %s)' % (row.id, k, name)
        if nb == 0:
            assert bool((scratch.view() == byte).all()), '%s: a call whose query is 0 wrote its scratch (fill %s)' % (row.id, name)
        for k, v in outs.items():
            if v.is_floating_point():
                assert bool(torch.isfinite(v).all()), '%s: %d non-finite elements in `%s` (fill %s)' % (row.id, int((~torch.isfinite(v)).sum()), k, name)
        for k, v in spec['ins'].items():
            assert same_bits(ins[k].view(v.dtype, tuple(v.shape)).cpu(), v), '%s: input `%s` was modified (fill %s)' % (row.id, k, name)
        results.append({k: v.cpu() for k, v in outs.items()})
        if operands:
            spec['check'](results[-1])
    for (name, _), got in zip(fills[1:], results[1:]):
        for k in got:
            assert same.get(k, same_bits)(got[k], results[0][k]), '%s: fill %s changes `%s`: %d of %d elements differ' % (
                row.id, name, k, int((got[k] != results[0][k]).sum()), got[k].numel())
    if not operands:
        spec['check'](results[0])
    return results
