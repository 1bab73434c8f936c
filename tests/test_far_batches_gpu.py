"""Far offsets and long batches through the device-resident entry points (tests/_far_batches.py has the cases and why; the worker,
tests/_far_batches_worker.py, what a child does): inputs and outputs past 2^31 and 2^32 bytes, and batches of more frames than the 65535
blocks of grid.y / grid.z, so that for_each_chunk (csrc/bevw_host.h) cuts k_vsum, k_gain, k_channel_sums, the per-pixel stitch and
remap_launch at least once.  One child per case, each with a time limit of its own; a child that dies ends the session (run_child).

What is cut where.  A balance handle on the PER-PIXEL schedule keeps the whole batch in one vsum_launch / k_gain / k_channel_sums, so at
92,376 frames all three are cut at 65535 -- k_vsum inside frame set 16383.  On the PLAN schedule balance_plan_run slices the batch in two
(46,188 frames each), so k_vsum is NOT cut there, and neither is the gain pass; those cases cover the far bases of the slices' scratch
(`tmp`, `pre`) and of the output, not the cut.  k_shard_pp's grid.z cut is not exercised either (camera shards are out of scope here).

The one-channel kernels and the moving stitch have cases of their own (tests/test_batch_loops_gpu.py runs their batch loops below 4 GiB):
BevGenerator(channels=1) on T at 62,000 bytes per image -- 69,276 frame sets, past 2^32 output bytes AND past one grid of images, so the
bases of k_stitch_units_gray (plan) and the cut of k_stitch_pp_gray (per_pixel) are both met; 16-bit linear and nearest remappers at
124,000 bytes per image on the units (the `* 2u` of k_units_gray16 / k_units_nn16 on offsets past 2^32); 65,540 small 16-bit linear and
8-bit nearest images with the plan off (remap_launch's cut on k_remap_lut_gray16 / k_remap_nn8); and 65,540 frame sets through
bevw_run_homographies_device, set b on rig b % 7 (the launcher's second span and its `minv + b0 * 36`).

The expected images are the oracle's on the pool's seven frame sets, computed once per geometry, format and mode here in the parent.  A
case skips only when the child reports that bevw_malloc returned BEVW_E_NOMEM (the balance cases peak near 10 GB of HBM).

Time limits: about five times the wall time measured per child (profiles/f16_addresses/durations.txt), never below 60 s."""
import numpy as np
import pytest

from tests import _batch_loops as BL
from tests import _caller_maps as CM
from tests import _far_batches as FB
from tests import _gray_stitch as GS
from tests import _moving as MV
from tests import _nearest as N
from tests import _nv12_out_spec as SO
from tests._harness import outside_of, run_child, uncovered

pytestmark = pytest.mark.gpu

CASES = FB.cases()
# seconds per child: every child measured between 0.6 and 1.3 s of wall time (profiles/f16_addresses/durations.txt), so five times that
# lies under the floor of 60 s for all of them; the margin covers a cold code-object load and a busy shared box
TIMEOUT = {c.name: 60 for c in CASES}

_want = {}


def stitch_expectation(oracle, c):
    key = (c.geometry, c.inp, c.mode)
    if key not in _want:
        cfg, _ = FB.GEOMETRIES[c.geometry]
        native, back, car = FB.pool(cfg, c.inp)
        ref = oracle.RefBevGenerator(FB.scaled_rig(cfg), cfg, *FB.MODES[c.mode])
        none = uncovered(ref)
        assert none.any()
        want = np.stack([ref(*back[k], car) for k in range(FB.POOL)])
        assert len({w.tobytes() for w in want}) == FB.POOL, "two pool sets give the same image"
        _want[key] = (native, car, want, none)
    return _want[key]


def gray_expectation(oracle, c):
    """channels=1 on the case's geometry, direct: tests/_gray_stitch.spec over the oracle on the grey pool"""
    if "gray" not in _want:
        cfg, _ = FB.GEOMETRIES[c.geometry]
        pool, car = FB.gray_pool(cfg)
        ref = oracle.RefBevGenerator(FB.scaled_rig(cfg), cfg, blend=False)
        none = uncovered(ref)
        want = GS.spec_batch(oracle, ref, pool, car)
        assert none.any() and len({w.tobytes() for w in want}) == FB.POOL, "two pool sets give the same image"
        _want["gray"] = dict(pool=pool, car=car, want=want, none=none)
    return _want["gray"]


def moving_expectation(oracle):
    """frame set k of the pool through RefBevGenerator(rig k of the seven perturbed rigs), direct, with the car"""
    cfg = FB.MOVING_CFG
    rigs = BL.moving_rigs(oracle, cfg)
    assert len(rigs) == FB.MOVING_RIGS == FB.POOL
    pool, _, car = FB.pool(cfg, "bgr")
    refs = [oracle.RefBevGenerator(r, cfg, blend=False) for _, r in rigs]
    want = np.stack([refs[k](*pool[k], car) for k in range(FB.POOL)])
    same_rig = np.stack([refs[0](*pool[k], car) for k in range(FB.POOL)])
    assert len({w.tobytes() for w in want}) == FB.POOL and all(not np.array_equal(want[k], same_rig[k]) for k in range(1, FB.POOL)), "a wrong matrix would pass"
    return dict(pool=pool, car=car, want=want, none=np.all([uncovered(ref) for ref in refs], axis=0), table=MV.table(rigs))


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_far_case(oracle, tmp_path, name):
    c = FB.case(name)
    case_file = str(tmp_path / "case.npz")
    if c.kind == "stitch":
        native, car, want, none = stitch_expectation(oracle, c)
        np.savez(case_file, pool=native, car=car, want_bgr=want, none=none, want=SO.bgr_to_nv12(want) if c.out == "nv12" else want)
    elif c.kind == "stitch_gray":
        np.savez(case_file, **gray_expectation(oracle, c))
    elif c.kind in ("plane", "plane_count"):
        size, family = (FB.REMAP_SIZE, FB.REMAP_FAMILY) if c.kind == "plane" else (FB.COUNT_SIZE, FB.COUNT_FAMILY)
        pool = FB.plane_pool(size, c.depth)
        m1, m2 = CM.family(family, *size)
        if c.nearest:
            want, fixed = N.want_nn(pool, m1, m2), ~N.inside_nn(m1, m2, size[0], size[1])
        else:
            want, fixed = np.stack([oracle.remap(f, m1, m2) for f in pool]), outside_of(m1, size[0], size[1])
        assert want.dtype == pool.dtype and len({w.tobytes() for w in want}) == FB.POOL and fixed.any() and not fixed.all()
        np.savez(case_file, pool=pool, want=want, fixed=fixed)
    elif c.kind == "moving":
        np.savez(case_file, **moving_expectation(oracle))
    else:
        size, family = (FB.REMAP_SIZE, FB.REMAP_FAMILY) if c.kind == "remap" else (FB.COUNT_SIZE, FB.COUNT_FAMILY)
        pool = FB.remap_pool(size)
        m1, m2 = CM.family(family, *size)
        want = np.stack([oracle.remap(f, m1, m2) for f in pool])
        assert len({w.tobytes() for w in want}) == FB.POOL
        np.savez(case_file, pool=pool, want=want)
    p = run_child("_far_batches_worker.py", [case_file, name], c.env, ("BEVW_REMAP_PLAN",), TIMEOUT[name], "far worker done")
    skipped = [l for l in p.stdout.splitlines() if l.startswith("SKIPPED:")]
    if skipped:
        assert "BEVW_E_NOMEM" in skipped[0], skipped[0]
        pytest.skip(skipped[0])
    assert "worker OK %s" % name in p.stdout, p.stdout[-2000:]
