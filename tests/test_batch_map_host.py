"""Who writes which frames of a batch, checked WITHOUT a GPU for every batch size.

tests/native/batch_map_exhaustive.cpp compiles plan_args, plan_grid, plan_block_map (cameracalibration_amd/csrc/bevw_plan.h) and
xcd_frame_map / xcd_frame_grid (bevw_device.h) for the host and enumerates batches 1 .. 520 x explicit frames per block 0 (default) .. 33
x the three XCD maps x group counts {1, 2, 7, 64}: over the block ids of the launch every (chunk, group) pair exactly once (a duplicate is
a second writer of a unit, a gap a stale image region), every other id rejected, the chunks' frame ranges non-empty and tiling the batch;
the same for the per-frame kernels' map.  The GPU batch tests (tests/test_batch_chunks_gpu.py) sample eight batch sizes, chosen by a table
of chunk shapes: that table is held against the library's own plan_args here, so a change of the nb heuristic flags the list as stale."""
import os
import shutil
import subprocess

import pytest

from tests import _harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests import _native_build

    out = str(tmp_path_factory.mktemp("batch_map") / "batch_map_exhaustive")
    _native_build.build(os.path.join(ROOT, "tests", "native", "batch_map_exhaustive.cpp"), out)
    return out


def test_every_block_map_is_complete_and_without_duplicates(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan block map ok: %d cases" % (520 * 34 * 3 * 4) in r.stdout, r.stdout
    assert "frame map ok: %d cases" % (3 * 520) in r.stdout, r.stdout


def plan_args(exe, batches):
    """batch -> (nb, chunks, frames of the last chunk, XCD map in use, idle chunk slots) as the library's plan_args / plan_grid give them."""
    r = subprocess.run([exe, "--plan-args"] + [str(b) for b in batches], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert [row[0] for row in rows] == list(batches)
    return {row[0]: row[1:] for row in rows}


def test_gpu_batch_sizes_have_the_chunk_shapes_they_were_chosen_for(exe):
    assert sorted(H.PLAIN) == sorted(H.SLICES) == sorted(H.BATCHES)
    got = plan_args(exe, sorted(H.BATCHES))
    assert got == H.PLAIN, "the nb heuristic changed: choose the batch sizes of tests/test_batch_chunks_gpu.py again"
    # what the list is for: nb of 1, 2, 3, 8 and 16; ragged chunks of more than one frame; odd full chunks; an XCD-affine launch with idle
    # chunk slots and one whose chunk count is no multiple of 8; the chunk-major map
    assert {v[0] for v in got.values()} == {1, 2, 3, 8, 16}
    assert any(nb > 2 and 1 < last < nb for nb, _, last, _, _ in got.values())
    assert any(nb % 2 == 1 and nb > 1 and last < nb for nb, _, last, _, _ in got.values())
    assert any(aff == 1 and n % 8 != 0 and idle > 0 for _, n, _, aff, idle in got.values()) and any(aff == 0 for _, _, _, aff, _ in got.values())
    # balance handles: the slices of balance_plan_run, each with a chunk size of its own
    for batch, slices in H.SLICES.items():
        sizes = H.balance_slices(batch)
        assert sizes == [s[0] for s in slices] and sum(sizes) == batch, batch
        per = plan_args(exe, sizes)
        assert [(n,) + per[n][:3] for n in sizes] == list(slices), batch
