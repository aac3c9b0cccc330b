"""Guarded device buffers for the scratch / workspace contract tests (a plain helper module).

`Guarded(nbytes, fill, dev, band)` is ONE uint8 allocation laid out as [front band | payload | back band]: the payload starts
256-byte aligned, the bands are multiples of 256 bytes, and every byte of all three holds `fill`.  A kernel that writes one byte
outside the payload changes a band (`intact()`), a kernel that reads outside it reads the fill (NaN for tensors), and a kernel that
reads its scratch before writing it sees whatever `fill` says the memory held before:

  Z  0x00  zeros: what a fresh allocation usually is (the baseline)
  N  0xFF  every fp32 / fp64 word a NaN, every int32 -1: reads that propagate
  F  0x4B  every fp32 ~ 1.3e7, every fp64 ~ 1e55, every int32 ~ 1.3e9, all finite: reads that a NaN-dropping op (fmaxf, clamps,
           selects) or a counter would hide from N

Bands are 1 MiB for workspaces and scratch, 16 KiB (the 4096 floats of the older guarded tests) for tensors."""
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


def tensor_in(t, dev, band=TENSOR_BAND):
    """A guarded device copy of the CPU tensor `t` (contiguous) with NaN bands: a read outside it shows up in a result.
    Returns (Guarded, device view)."""
    t = t.contiguous()
    g = Guarded(t.numel() * _item(t.dtype), N, dev, band)
    v = g.view(t.dtype, tuple(t.shape))
    v.copy_(t)
    return g, v


def tensor_out(shape, dev, dtype=torch.float32, band=TENSOR_BAND):
    """A guarded, NaN-filled output tensor: an element the call leaves unwritten shows up.  Returns (Guarded, device view)."""
    n = 1
    for s in shape:
        n *= int(s)
    g = Guarded(n * _item(dtype), N, dev, band)
    return g, g.view(dtype, tuple(shape))
