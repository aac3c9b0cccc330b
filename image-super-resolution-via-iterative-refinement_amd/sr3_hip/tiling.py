"""Tile layout of tiled sampling: where the overlapping tiles of an image lie and how their predictions are weighted.

Pure Python / numpy, no device.  An image larger than the size the UNet was trained at is sampled as ONE chain whose eps comes from
overlapping tiles of the training size (EngineDiffusion.p_sample_loop_tiled); this module decides the tiles and the blend weights,
csrc/tiled.hip applies them.

Tiling (engine extension, `"tiling": {"tile": 128 | [th, tw], "overlap": 32, "batch": 8}` next to "sampler", or `set_tiling`): an image larger
than the tile is sampled as one chain whose eps comes from overlapping tiles of that size -- per step: sr3_tile_gather + UNet forward
per chunk of tiles, then sr3_tiled_step (blend + p_sample update + counter decrement) on the whole image (`p_sample_loop_tiled`).
"""
import numpy as np


def _as_int(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError('tiling: %s must be an integer (got %r)' % (what, v))
    return int(v)


def axis_origins(L, t, o):
    """Origins of the tiles of size t along an axis of length L with at least o pixels of overlap between neighbours (0 <= o < t).
    L <= t: one tile (of size L) at 0.  Else n = ceil((L - o) / (t - o)) tiles at (k * (L - t)) // (n - 1): the first at 0, the last at
    L - t, strictly increasing, and since (L - t) / (n - 1) <= t - o consecutive tiles overlap by at least o.  Integer arithmetic only;
    the origins are not aligned to anything."""
    L, t, o = _as_int(L, 'the axis length'), _as_int(t, 'the tile size'), _as_int(o, 'the overlap')
    if L <= 0 or t <= 0:
        raise ValueError('tiling: axis length and tile size must be positive (got %d, %d)' % (L, t))
    if not 0 <= o < t:
        raise ValueError('tiling: the overlap must lie in [0, tile) (got overlap %d, tile %d)' % (o, t))
    if L <= t:
        return [0]
    n = -((L - o) // -(t - o))
    return [(k * (L - t)) // (n - 1) for k in range(n)]


def axis_window(t, o):
    """Separable blend weight of a tile along one axis: w[i] = min(1, (i + 1) / (o + 1), (t - i) / (o + 1)), fp32 from float64.
    Strictly positive, a linear ramp across the overlap, all ones for o = 0."""
    t, o = _as_int(t, 'the tile size'), _as_int(o, 'the overlap')
    if t <= 0 or o < 0:
        raise ValueError('tiling: window of tile %d, overlap %d' % (t, o))
    i = np.arange(t, dtype=np.float64)
    return np.minimum(1.0, np.minimum((i + 1.0) / (o + 1.0), (t - i) / (o + 1.0))).astype(np.float32)


def parse_tile(tile):
    """tile: an int (square) or a pair (th, tw) -> (th, tw), positive integers."""
    if isinstance(tile, (list, tuple)):
        if len(tile) != 2:
            raise ValueError('tiling: "tile" must be an integer or a pair [th, tw] (got %r)' % (tile,))
        th, tw = _as_int(tile[0], 'the tile height'), _as_int(tile[1], 'the tile width')
    else:
        th = tw = _as_int(tile, 'the tile size')
    if th <= 0 or tw <= 0:
        raise ValueError('tiling: the tile size must be positive (got %d x %d)' % (th, tw))
    return th, tw


class TileGrid(object):
    """The tiles of an H x W image: origins per axis (oy, ox), the effective tile size (th, tw) = min(tile, L) per axis, the two
    blend windows (wy, wx), n_tiles = ny * nx.  Tile order: row-major within an image, the image index outermost --
    tile_index(b, iy, ix) = (b * ny + iy) * nx + ix.  `divisor`: what the UNet's halvings need the tile size to be a multiple of.
    The overlap must be smaller than BOTH sides of the nominal tile, whatever the image: a rectangular tile is refused for an overlap its
    short side cannot hold even where that axis ends up with a single tile (the same rule as parse_tiling, which has no image to ask)."""

    def __init__(self, H, W, tile_h, tile_w, overlap, divisor=1):
        H, W = _as_int(H, 'the image height'), _as_int(W, 'the image width')
        tile_h, tile_w = parse_tile((tile_h, tile_w))
        overlap, divisor = _as_int(overlap, 'the overlap'), _as_int(divisor, 'the divisor')
        if H <= 0 or W <= 0:
            raise ValueError('tiling: the image size must be positive (got %d x %d)' % (H, W))
        if overlap < 0 or overlap >= min(tile_h, tile_w):
            raise ValueError('tiling: the overlap must lie in [0, tile) (got overlap %d, tile %d x %d)' % (overlap, tile_h, tile_w))
        self.H, self.W, self.overlap = H, W, overlap
        self.th, self.tw = min(tile_h, H), min(tile_w, W)
        if divisor < 1 or self.th % divisor or self.tw % divisor:
            raise ValueError('tiling: tile size %d x %d: height and width must be multiples of %d (the UNet\'s halvings)'
                             % (self.th, self.tw, divisor))
        # (an axis the tile covers has one tile and no overlap: its window is all ones)
        self.oy = axis_origins(H, tile_h, overlap)
        self.ox = axis_origins(W, tile_w, overlap)
        self.ny, self.nx = len(self.oy), len(self.ox)
        self.n_tiles = self.ny * self.nx
        self.wy = axis_window(self.th, overlap if self.ny > 1 else 0)
        self.wx = axis_window(self.tw, overlap if self.nx > 1 else 0)

    def tile_index(self, b, iy, ix):
        return (b * self.ny + iy) * self.nx + ix

    def tile_of(self, index):
        """(b, iy, ix) of a global tile index."""
        b, r = divmod(int(index), self.n_tiles)
        return (b,) + divmod(r, self.nx)

    def slices(self, iy, ix):
        return slice(self.oy[iy], self.oy[iy] + self.th), slice(self.ox[ix], self.ox[ix] + self.tw)


def parse_tiling(spec, divisor=1):
    """The "tiling" block of a beta_schedule phase -> None (absent / null) or a dict {tile: (th, tw), overlap, batch}.
    {"tile": 128 | [th, tw], "overlap": 32, "batch": 8}; overlap defaults to 0, batch to None (all tiles, at most 16).
    One overlap serves both axes, so it must be smaller than both th and tw."""
    if spec is None:
        return None
    if not hasattr(spec, 'get'):
        raise ValueError('tiling: a mapping {"tile", "overlap", "batch"} is expected (got %r)' % (spec,))
    if spec.get('tile') is None:
        raise ValueError('tiling: "tile" is required')
    th, tw = parse_tile(spec['tile'])
    overlap = _as_int(spec.get('overlap', 0) or 0, 'the overlap')
    if overlap < 0 or overlap >= min(th, tw):
        raise ValueError('tiling: the overlap must lie in [0, tile) (got overlap %d, tile %d x %d)' % (overlap, th, tw))
    if th % divisor or tw % divisor:
        raise ValueError('tiling: tile size %d x %d: height and width must be multiples of %d (the UNet\'s halvings)' % (th, tw, divisor))
    batch = spec.get('batch')
    if batch is not None:
        batch = _as_int(batch, 'the tile batch')
        if batch < 1:
            raise ValueError('tiling: the tile batch must be positive (got %d)' % batch)
    return dict(tile=(th, tw), overlap=overlap, batch=batch)
