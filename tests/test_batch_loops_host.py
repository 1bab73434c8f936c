"""The host leg of the batch-loop tests (tests/_batch_loops.py, tests/test_batch_loops_gpu.py) -- WITHOUT a GPU.

  * moving_nb (csrc/bevw_moving.h) compiled for the host (tests/native/batch_loops_census.cpp): the table the GPU batches of
    k_stitch_moving were chosen by, and batches 1 .. 520 x tile counts {1, 252, 4096, 73170} -- every frame set in exactly one block;
  * the remappers' map through the library's own plan compiler: units without a contributor and per-tap base tiles both exist (and the
    fisheye map of the front camera, which the issue of these tests named first, has neither);
  * the pools: all 143 expected images pairwise distinct in every form, so that a wrong frame cannot pass;
  * a negative control: the images a wrong frame_of() clamp leaves fail the comparer for every batch of H.BATCHES whose chunks hold more
    than one frame, by the name of the frame."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _batch_loops as BL
from tests import _harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests import _native_build

    out = str(tmp_path_factory.mktemp("batch_loops") / "batch_loops_census")
    _native_build.build(os.path.join(ROOT, "tests", "native", "batch_loops_census.cpp"), out)
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


# ---------------------------------------------------------------------------------------------------------------
# moving_nb
# ---------------------------------------------------------------------------------------------------------------
@needs_hipcc
def test_every_frame_set_lies_in_exactly_one_block(exe):
    assert "moving blocks ok: %d cases" % (520 * 4) in run(exe, "--moving-nb")


@needs_hipcc
def test_moving_batches_have_the_blocks_they_were_chosen_for(exe):
    cfg = BL.MOVING_CFG
    assert BL.MOVING_TILES == -(-cfg["BEV_WIDTH"] // 64) * -(-cfg["BEV_HEIGHT"] // 4) == 252
    assert sorted(BL.MOVING) == sorted(BL.MOVING_BATCHES) and BL.MOVING_POOL == 259
    rows = [tuple(int(v) for v in line.split()) for line in run(exe, "--moving-table", BL.MOVING_TILES, *sorted(BL.MOVING)).splitlines()]
    got = {r[0]: r[1:] for r in rows}
    assert got == BL.MOVING, "moving_nb changed: choose the batches of tests/test_batch_loops_gpu.py again"
    assert {4, 8, 16} <= {nb for nb, _, _ in got.values()}
    for B in BL.MOVING_BATCHES[:3]:
        nb, blocks, last = got[B]
        assert nb in (4, 8, 16) and 1 < last < nb and blocks > 1, (B, got[B])   # a ragged last block of more than one frame set
    assert BL.MOVING_BATCHES[3:] == (33, 9) and got[33][0] == 2 and got[9][0] == 1   # ... then shrinking, down to one set per block
    # what the existing cases of tests/test_moving_gpu.py run on the small rig's 252 tiles: one set per block up to batch 32, two at 33
    small = [tuple(int(v) for v in line.split()) for line in run(exe, "--moving-table", 252, 1, 5, 17, 32, 33).splitlines()]
    assert [r[1] for r in small] == [1, 1, 1, 1, 2]
    assert len(BL.MOVING_RIGS) == 7 and all(np.gcd(7, nb) == 1 for nb, _, _ in got.values())


# ---------------------------------------------------------------------------------------------------------------
# the remappers: a census of the map through the plan compiler, and of the pools through the yardsticks
# ---------------------------------------------------------------------------------------------------------------
def units_census(exe, tmp_path, maps, name):
    sw, sh, dw, dh = BL.REMAP_SIZE
    p = str(tmp_path / (name + ".bin"))
    with open(p, "wb") as f:
        f.write(struct.pack("<4i", sw, sh, dw, dh))
        f.write(np.ascontiguousarray(maps[0], np.int16).tobytes())
        f.write(np.ascontiguousarray(maps[1], np.uint16).tobytes())
    words = run(exe, "--units", p).split()
    assert words[0::2] == ["units", "empty", "tiles", "per_tap"], words
    return dict(zip(words[0::2], (int(v) for v in words[1::2])))


@needs_hipcc
def test_the_remappers_map_has_units_without_a_contributor_and_per_tap_tiles(exe, tmp_path, oracle):
    got = units_census(exe, tmp_path, BL.remap_maps(), "map")
    print(BL.REMAP_FAMILY, got)
    assert got["units"] > 1 and got["empty"] > 0 and got["per_tap"] > 0 and got["empty"] < got["units"] and got["tiles"] == 20 * 64
    front = units_census(exe, tmp_path, BL.front_maps(oracle), "front")
    print("front camera", front)
    assert front["empty"] == 0 and front["per_tap"] == 0, "the front camera's own map has them now: BL.REMAP_FAMILY may go"


@pytest.mark.parametrize("kind,depth", BL.REMAPPERS, ids=["%s%d" % r for r in BL.REMAPPERS])
def test_expected_images_are_pairwise_distinct(oracle, kind, depth):
    frames = BL.remap_frames(depth)
    assert frames.shape[0] == BL.POOL and frames.dtype == BL.DTYPE[depth] and frames.max() == (1 << depth) - 1 and frames.min() == 0
    want, fixed = BL.remap_want(oracle, kind, frames, BL.remap_maps())
    assert want.dtype == frames.dtype and fixed.any() and (~fixed).sum() > 50000 and not want[:, fixed].any()
    assert len({w.tobytes() for w in want}) == BL.POOL, "two frames of the pool give the same image"
    if depth == 16:   # ... and no image is told from another by one byte of its pixels alone
        assert len({(w >> 8).tobytes() for w in want}) == BL.POOL and len({(w & 255).tobytes() for w in want}) == BL.POOL


# ---------------------------------------------------------------------------------------------------------------
# the negative control
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def control(oracle):
    frames = BL.remap_frames(8)
    return BL.remap_want(oracle, "linear", frames, BL.remap_maps())


def compare(images, want, fixed, B):
    for b in range(B):
        H.check_plane(images[b], want[b], fixed, "control, %s" % H.where(B, b))


@pytest.mark.parametrize("B", H.BATCHES)
def test_a_wrong_clamp_fails_the_comparer(control, B):
    want, fixed = control
    nb = H.PLAIN[B][0]
    compare(want[:B], want, fixed, B)
    bad = BL.wrong_clamp(want[:B], nb)
    if nb == 1:   # one frame per chunk: the ring's step past the chunk IS the next chunk's frame -- nothing to tell apart
        return
    assert not np.array_equal(bad, want[:B])
    with pytest.raises(AssertionError, match=r"batch %d, frame %d: chunk 1 \(%d frames per chunk\), %s of its chunk.*pixels differ" % (
            B, nb, nb, "the LAST frame" if B - nb == 1 else "not the last frame")):
        compare(bad, want, fixed, B)
    # ... and with the batch's last image alone wrong (a ragged last chunk that wrote its first frame twice)
    last = want[:B].copy()
    last[B - 1] = want[B - 2]
    with pytest.raises(AssertionError, match="batch %d, frame %d: .*the LAST frame" % (B, B - 1)):
        compare(last, want, fixed, B)


def test_check_plane_controls():
    want = np.random.default_rng(3).integers(1, 65536, (8, 16), dtype=np.uint16)
    fixed = np.zeros((8, 16), bool)
    fixed[:, :4] = True
    want[fixed] = 0
    H.check_plane(want.copy(), want, fixed, "equal")
    for at, word in (((5, 9), "pixels differ"), ((2, 1), "no frame reaches")):
        got = want.copy()
        got[at] += 1
        with pytest.raises(AssertionError, match=word):
            H.check_plane(got, want, fixed, "one pixel + 1")
    with pytest.raises(AssertionError):
        H.check_plane(want.astype(np.uint8), want, fixed, "dtype")
    with pytest.raises(AssertionError):
        H.check_plane(want[:-1], want, fixed, "shape")
    car = np.full((8, 16), 77, np.uint16)
    with pytest.raises(AssertionError, match="are not the car"):
        H.check_plane(want.copy(), want, fixed, "zeros under the car", under=car)
    under = np.where(fixed, car, want)
    H.check_plane(under.copy(), under, fixed, "the car", under=car)
    raw = np.arange(2 * 8 * 20, dtype=np.uint8)
    assert H.plane_of(raw, np.uint16, 8, 8, 20).shape == (8, 8) and H.plane_of(raw, np.uint8, 16, 16, 20)[1, 0] == 20
    assert H.where(67, 64, nb_env={67: 4}) == "batch 67, frame 64: chunk 16 (4 frames per chunk), not the last frame of its chunk"
    assert "the LAST frame" in H.where(67, 66, nb_env={67: 4}) and "chunk 0 (16 frames per chunk)" in H.where(143, 3)
