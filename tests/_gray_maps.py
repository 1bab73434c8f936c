"""A caller-made map for the one-channel remapper's tests that tests/_caller_maps.py does not hold: a smooth shift whose footprints END in
the frame's last texel.

edge_shift(sw, sh, dw, dh): destination (x, y) samples (sw - 1 - dw + x, sh - 1 - dh + y) with a uniform random map2, so the bottom-right
pixel's footprint is texels (sw - 2 .. sw - 1, sh - 2 .. sh - 1): interior by one texel, its bottom row the frame's last row and its
right column inside the LAST 4-texel group of that row -- the group whose 8-byte load would reach a dword past the frames."""
import numpy as np


def edge_shift(sw, sh, dw, dh, seed=31):
    assert sw > dw and sh > dh
    y, x = np.mgrid[0:dh, 0:dw]
    m1 = np.stack([sw - 1 - dw + x, sh - 1 - dh + y], -1).astype(np.int16)
    m2 = np.random.default_rng(seed).integers(0, 65536, (dh, dw)).astype(np.uint16)
    return np.ascontiguousarray(m1), np.ascontiguousarray(m2)
