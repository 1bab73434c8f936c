"""NV12 frames laid out in device memory the way decoders leave them: every frame a SURFACE -- a Y plane and a U / V plane with a row pitch,
each at an address of its own -- inside ONE arena allocated for the purpose.  Test infrastructure for bevw_run_surfaces_device,
bevw_run_surface_table_device and bevw_remap_surfaces_device.

Nothing here places a plane at the edge of the allocation or points a table outside it: the arena starts and ends with a margin, every
plane lies wholly inside it, and the gaps and padding columns hold random bytes (from a seed of their own) so that a kernel which lets a
byte outside the FW x FH texels into a result is caught by comparing two arenas that differ only there."""
import numpy as np

MARGIN = 4096   # bytes in front of the first and behind the last plane


def plane_sizes(fh: int, pitch: int):
    return pitch * fh, pitch * fh // 2


def layout(n: int, fh: int, pitch: int, rng: np.random.Generator, mode: str = "shuffled"):
    """Byte offsets (y_off[n], uv_off[n]) of the planes of n surfaces and the arena size.
    'shuffled': all 2n planes in random order with gaps of varying size (multiples of 4 bytes, 4 .. 8 KB);
    'split':    the U / V planes in a region of their own BETWEEN two halves of the Y planes, every region shuffled: uv - y differs per
                surface and is negative for the surfaces of the second half;
    'packed':   surface k at k * pitch * fh * 3 / 2, U / V right behind Y, no gaps (what a dense frame set is when pitch == FW)."""
    ysz, csz = plane_sizes(fh, pitch)
    y_off, uv_off = np.zeros(n, np.int64), np.zeros(n, np.int64)
    if mode == "packed":
        for k in range(n):
            y_off[k] = MARGIN + k * (ysz + csz)
            uv_off[k] = y_off[k] + ysz
        return y_off, uv_off, MARGIN + n * (ysz + csz) + MARGIN
    if mode == "shuffled":
        order = [("y", k) for k in range(n)] + [("uv", k) for k in range(n)]
        order = [order[i] for i in rng.permutation(len(order))]
    elif mode == "split":
        ys = [("y", int(k)) for k in rng.permutation(n)]
        order = ys[:n // 2] + [("uv", int(k)) for k in rng.permutation(n)] + ys[n // 2:]
    else:
        raise ValueError(mode)
    pos = MARGIN
    for kind, k in order:
        pos += 4 * int(rng.integers(1, 2049))
        if kind == "y":
            y_off[k] = pos
            pos += ysz
        else:
            uv_off[k] = pos
            pos += csz
    return y_off, uv_off, pos + MARGIN


def fill(arena: np.ndarray, frames: np.ndarray, fw: int, fh: int, pitch: int, y_off, uv_off) -> None:
    """Write NV12 frames [n, fh * 3 // 2, fw] into the arena as surfaces with rows of `pitch` bytes (padding columns are left as they are)."""
    n = frames.shape[0]
    ysz, csz = plane_sizes(fh, pitch)
    for k in range(n):
        assert MARGIN <= y_off[k] and y_off[k] + ysz <= arena.size - MARGIN and MARGIN <= uv_off[k] and uv_off[k] + csz <= arena.size - MARGIN
        arena[y_off[k]:y_off[k] + ysz].reshape(fh, pitch)[:, :fw] = frames[k, :fh]
        arena[uv_off[k]:uv_off[k] + csz].reshape(fh // 2, pitch)[:, :fw] = frames[k, fh:]


class Surfaces:
    """n NV12 frames resident in one device arena as surfaces.  `.table` is uint64 [n, 2] (device addresses of Y and U / V), `.arena` the
    device buffer (free() when done), `.host` the arena's bytes."""

    def __init__(self, ffi, frames: np.ndarray, fw: int, fh: int, pitch: int, layout_seed: int = 1, fill_seed: int = 2, mode: str = "shuffled"):
        frames = np.asarray(frames)
        assert frames.dtype == np.uint8 and frames.ndim == 3 and frames.shape[1:] == (fh * 3 // 2, fw), frames.shape
        assert pitch >= fw and pitch % 4 == 0
        n = frames.shape[0]
        y_off, uv_off, size = layout(n, fh, pitch, np.random.default_rng(layout_seed), mode)
        self.host = np.frombuffer(np.random.default_rng(fill_seed).bytes(size), np.uint8).copy()   # gaps and padding columns: random bytes
        fill(self.host, frames, fw, fh, pitch, y_off, uv_off)
        self.arena = ffi.DeviceBuffer(size).upload(self.host)
        self.y_off, self.uv_off = y_off, uv_off
        self.table = np.stack([self.arena.ptr + y_off, self.arena.ptr + uv_off], axis=1).astype(np.uint64)
        assert (self.table % 4 == 0).all()

    def free(self):
        self.arena.free()
