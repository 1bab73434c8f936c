"""The NV12 input path checked WITHOUT a GPU.

tests/native/nv12_exhaustive.cpp compiles the kernels' own conversion (bevw_device.h: nv12_row_bgr), the landing of one NV12 texel group
into the four pair entries of the unit kernel's LDS patch (bevw_pair.h: pair_convert_nv12) and the host translation of a unit's group list
into NV12 offsets (bevw_unit.h: unit_gsrc_nv12) for the host.  Their results are compared here with the NumPy specification
(tests/_nv12_spec.py): the conversion over all 2^24 (Y, U, V) triples, the landing against pair entries built from the specification's BGR
texels, the offsets against the bytes they must address."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import _nv12_spec as S

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
NO_GROUP = 0x80000000   # kPairNoGroup (bevw_pair.h)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests import _native_build

    path = str(tmp_path_factory.mktemp("nv12") / "nv12_exhaustive")
    _native_build.build(os.path.join(ROOT, "tests", "native", "nv12_exhaustive.cpp"), path)
    return path


def test_conversion_of_every_yuv_triple(exe, tmp_path):
    out = str(tmp_path / "table.bin")
    r = subprocess.run([exe, "table", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, np.uint8).reshape(256, 256, 256, 3)
    i = np.arange(256, dtype=np.uint8)
    want = S.yuv_to_bgr(i[:, None, None], i[None, :, None], i[None, None, :])
    bad = np.argwhere(np.any(got != want, axis=-1))
    assert bad.size == 0, "first mismatches (Y, U, V): %s" % bad[:5].tolist()
    # the value a lane without a group must NOT land: the conversion of the zeros a masked load returns
    assert want[0, 0, 0].tolist() == [0, 154, 0]


def _land(exe, tmp_path, fw, fh, ncams, frame_set, gsrc):
    paths = [str(tmp_path / n) for n in ("set.bin", "gsrc.bin", "offs.bin", "pairs.bin")]
    frame_set.tofile(paths[0])
    np.asarray(gsrc, np.uint32).tofile(paths[1])
    r = subprocess.run([exe, "land", str(fw), str(fh), str(ncams)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(paths[2], np.uint32).reshape(-1, 2), np.fromfile(paths[3], np.uint8).reshape(-1, 4, 8)


@pytest.mark.parametrize("fw,fh,ncams", [(16, 6, 4), (24, 10, 1), (8, 2, 4)])
def test_group_offsets_and_landing(exe, tmp_path, fw, fh, ncams):
    """Every group of a synthetic frame set -- the last of each row, the last of each frame and of the whole set among them -- and lanes
    without a group: the NV12 offsets address the group's Y and U / V bytes, and the landed pair entries are pair_convert's entries of the
    specification's BGR texels (zeros for a lane without a group)."""
    rng = np.random.default_rng(fw * 1000 + fh * 10 + ncams)
    nv_frame, gpr = fw * fh * 3 // 2, fw // 4
    frames = S.random_nv12(rng, (ncams,), fw, fh)
    ngroups = ncams * fh * gpr
    gsrc = [12 * k for k in range(ngroups)] + [NO_GROUP] * 3
    order = rng.permutation(len(gsrc))
    gsrc = [gsrc[i] for i in order]
    offs, pairs = _land(exe, tmp_path, fw, fh, ncams, frames.reshape(-1), gsrc)
    flat = frames.reshape(-1)
    bgr = S.nv12_to_bgr(frames)   # [ncams, fh, fw, 3]
    seen_row_end = seen_set_end = 0
    for slot, g in enumerate(gsrc):
        if g == NO_GROUP:
            assert offs[slot].tolist() == [NO_GROUP, NO_GROUP]
            assert not pairs[slot].any(), "a lane without a group must land zero pair entries"
            continue
        k = g // 12
        cam, rem = divmod(k, fh * gpr)
        y, x = rem // gpr, 4 * (rem % gpr)
        yo, co = int(offs[slot, 0]), int(offs[slot, 1])
        assert yo == cam * nv_frame + y * fw + x and co == cam * nv_frame + fw * fh + (y // 2) * fw + x
        assert np.array_equal(flat[yo:yo + 4], frames[cam, y, x:x + 4])
        assert np.array_equal(flat[co:co + 4], frames[cam, fh + y // 2, x:x + 4])
        for p in range(4):
            a, b = x + p, x + p + 1
            want = np.zeros(8, np.uint8)
            want[[0, 2, 4]] = bgr[cam, y, a]
            if b < fw:
                want[[1, 3, 5]] = bgr[cam, y, b]
                assert np.array_equal(pairs[slot, p], want), (slot, cam, y, x, p)
            else:   # texel x+4 of a row's last group lies outside the frame: no unit pixel samples it, its bytes are unspecified
                assert np.array_equal(pairs[slot, p, [0, 2, 4, 6, 7]], want[[0, 2, 4, 6, 7]]), (slot, cam, y, x, p)
        seen_row_end += x + 4 == fw
        seen_set_end += k == ngroups - 1
    assert seen_row_end == ncams * fh and seen_set_end == 1


def test_spec_helpers_round_trip():
    """The input generator of the GPU tests: grey stays (nearly) grey through BGR -> NV12 -> BGR."""
    img = np.full((4, 6, 3), 128, np.uint8)
    back = S.nv12_to_bgr(S.bgr_to_nv12(img))
    assert back.shape == img.shape and int(np.abs(back.astype(int) - 128).max()) <= 1
