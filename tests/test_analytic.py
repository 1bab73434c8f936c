"""Analytic projection mode (bevw_set_projection(BEVW_PROJ_ANALYTIC); SURVEY.md 8 row g1, BASELINE north star).

The reference's per-frame path is table-driven; this mode evaluates inverse homography + fisheye model per frame and pixel.
It is NOT the reference's arithmetic, so it is held to two different bars:
  * CPU: the fp64 NumPy specification (oracle/np_analytic.py) against the table path of the oracle on the reference's own
    frames -- the two must show the same picture (PSNR), which validates the projection formulas against the reference's
    tables; the differences are the tables' 1/32-pixel double quantisation (the LUT quirk), reported, not hidden.
  * GPU: the HIP kernel against that specification -- same formulas in fp64, so equal up to libm's atan / rounding ties:
    >= 99.9 % of the bytes identical, never more than 1 LSB apart.
The specification covers balance too (AnalyticBevGenerator(balance=True): the reference's chain around the analytic sample).  Every
kernel path of the mode -- full grid, left-over tiles, per pixel and frame, byte fetches and stores, balance, fp32 -- is held against
it in tests/test_analytic_gpu.py; the conditions those tests rest on (partial footprints on the shifted rig, the size of the fp32
edge band, gains far from 1, the measured fp32 position error and balance tie share) are checked here, on the CPU.
"""
import numpy as np
import pytest

from cameracalibration_amd import workloads as W
from tests._harness import SB, ffi  # noqa: F401


def psnr(a, b, sel=None):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    if sel is not None:
        d = d[sel]
    m = d.mean()
    return 99.0 if m == 0 else 10.0 * np.log10(255.0 ** 2 / m)


@pytest.mark.parametrize("blend", [False, True])
def test_specification_shows_the_same_picture_as_the_table_path(oracle, repo_rig, blend):
    from oracle import np_analytic

    cfg = dict(oracle.DEFAULT_CFG)
    frames = [repo_rig.image(n) for n in oracle.CAMERAS]
    ref = oracle.RefBevGenerator(repo_rig.rig, cfg, blend=blend, balance=False)(*frames)
    ana = np_analytic.AnalyticBevGenerator(repo_rig.rig, cfg, blend=blend)(*frames)
    assert ana.shape == ref.shape
    # pixels the table path fills from inside the undistorted image (outside it the tables hold the (0,0) quirk entries)
    inside = np.zeros(ref.shape[:2], bool)
    for i, n in enumerate(oracle.CAMERAS):
        _, _, valid = np_analytic.project(*repo_rig.rig[n], cfg)
        m = ref.shape and (oracle.direct_mask(n, cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], cfg["CAR_WIDTH"], cfg["CAR_HEIGHT"]) != 0)
        m = m if m.ndim == 2 else m[..., 0]
        inside |= valid & m
    p = psnr(ref, ana, inside)
    d = np.abs(ref.astype(np.int32) - ana.astype(np.int32))[inside]
    print("analytic vs table path, blend=%s: PSNR %.1f dB over %d pixels, mean |diff| %.2f, 99 %% <= %d LSB" % (
        blend, p, int(inside.sum()), d.mean(), int(np.percentile(d, 99))))
    assert inside.mean() > 0.5
    assert p > 38.0          # same picture (measured 43.7 / 44.2 dB); what is left is the tables' coordinate quantisation on the sample frames' edges
    assert d.mean() < 3.0


@pytest.mark.parametrize("blend", [False, True])
def test_balance_specification_shows_the_same_picture_as_the_table_path(oracle, repo_rig, blend):
    """the composition of AnalyticBevGenerator(balance=True) -- luminance balance of the frames, sample, mask, sums, white balance --
    against RefBevGenerator(balance=True) on the reference's own frames, at the bar of the unbalanced pair above"""
    from oracle import np_analytic

    cfg = dict(oracle.DEFAULT_CFG)
    frames = [repo_rig.image(n) for n in oracle.CAMERAS]
    ref = oracle.RefBevGenerator(repo_rig.rig, cfg, blend=blend, balance=True)(*frames)
    gen = np_analytic.AnalyticBevGenerator(repo_rig.rig, cfg, blend=blend, balance=True)
    ana = gen(*frames)
    inside = np.zeros(ref.shape[:2], bool)
    for n in oracle.CAMERAS:
        valid = np_analytic.project(*repo_rig.rig[n], cfg)[2]
        inside |= valid & (oracle.direct_mask(n, cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"], cfg["CAR_WIDTH"], cfg["CAR_HEIGHT"]) != 0)
    p = psnr(ref, ana, inside)
    d = np.abs(ref.astype(np.int32) - ana.astype(np.int32))[inside]
    pre = gen.pre_gain(*frames)
    k = np_analytic.gains(pre)
    print("analytic vs table path with balance, blend=%s: PSNR %.1f dB over %d pixels, mean |diff| %.2f, gains %s" % (
        blend, p, int(inside.sum()), d.mean(), k))
    assert ana.shape == ref.shape and inside.mean() > 0.5
    assert p > 38.0
    assert d.mean() < 3.0
    # the parts: the gains are color_balance's
    assert np.array_equal(oracle.color_balance(pre), ana)
    if oracle.get_variant(oracle.VARIANT_ADDWEIGHTED):
        assert np.array_equal(np.clip(np.rint(pre.astype(np.float64) * k), 0, 255).astype(np.uint8), ana)


@pytest.mark.parametrize("blend", [False, True])
def test_balance_specification_parts_on_the_small_rig(oracle, blend):
    """the car goes on after the gain, balance off is the unbalanced generator, the luminance shift is the oracle's"""
    from tests import _analytic_common as AC
    from oracle import np_analytic

    frames, car = AC.make_frames(1, cast=True)[0], AC.make_car()
    gen = AC.spec("small", blend=blend, balance=True)
    ana = gen(*frames)
    assert np.array_equal(gen(*frames, car), oracle.add_sat(ana, car)) and not np.array_equal(gen(*frames, car), ana)
    plain = np_analytic.AnalyticBevGenerator(AC.small_rig(), AC.SMALL_CFG, blend=blend)
    assert np.array_equal(gen.with_balance(False)(*frames, car), plain(*frames, car))
    assert np.array_equal(gen.pre_gain(*frames), plain(*oracle.luminance_balance(list(frames))))
    assert not np.array_equal(gen.pre_gain(*frames), plain(*frames))


# ---------------------------------------------------------------------------------------------------------------
# the conditions tests/test_analytic_gpu.py rests on, from the specification alone
# ---------------------------------------------------------------------------------------------------------------
def test_the_shifted_rig_has_partial_footprints_and_the_small_rig_none(oracle):
    """k_stitch_analytic on left-over tiles and the border branches of analytic_sample / k_stitch_perpixel run only where a footprint
    crosses the frame border: the shifted rig has such pixels (and thousands that sample nothing), the small rig none"""
    from tests import _analytic_common as AC

    for blend in (False, True):
        small, shifted = AC.footprint_census("small", blend=blend), AC.footprint_census("shifted", blend=blend)
        print("blend=%s (partial footprints, pixels that sample nothing) per camera: small rig %s, shifted rig %s" % (blend, small, shifted))
        assert sum(p for p, _ in small) == 0
        assert sum(p for p, _ in shifted) > 100 and sum(z for _, z in shifted) > 10000
    assert AC.footprint_census("shifted") == [(0, 0), (19, 8134), (204, 9928), (0, 0)]   # (the census this suite was written with)


@pytest.mark.parametrize("rig", ["small", "shifted"])
def test_fp32_position_error_is_the_recorded_one_and_the_edge_band_is_small(oracle, rig):
    """F32_EPS is measured: the projection in NumPy float32 against float64 on the test rigs, times 4.  The band it defines -- where the
    fp32 mode may decide validity the other way, and nothing is bounded -- holds at most 0.5 % of any camera's masked, valid pixels."""
    from tests import _analytic_common as AC

    e_uv, e_p, flips = AC.f32_position_error(rig)
    print("%s rig: float32 against float64 positions: |u, v| <= %.3g, |px, py| <= %.3g pixel, %d validity flips; F32_EPS = %.3g" % (
        rig, e_uv, e_p, flips, AC.F32_EPS))
    assert max(e_uv, e_p) <= AC.F32_POSITION_ERROR and AC.F32_EPS == 4 * AC.F32_POSITION_ERROR
    if rig == "shifted":
        assert max(e_uv, e_p) > 0.9 * AC.F32_POSITION_ERROR   # the recorded value is this rig's, not a round number above it
    for blend in (False, True):
        for cfg in (AC.SMALL_CFG, dict(AC.SMALL_CFG, BEV_WIDTH=250)):
            px, share = AC.band(rig, cfg, blend)
            print("%s rig, blend=%s, BW %d: %d band pixels, at most %.3f %% of a camera's masked, valid pixels" % (
                rig, blend, cfg["BEV_WIDTH"], int(px.sum()), 100 * share))
            assert share <= AC.BAND_CAP


@pytest.mark.parametrize("blend", [False, True])
@pytest.mark.parametrize("rig", ["small", "shifted"])
def test_balance_gains_are_far_from_one_and_the_tie_share_is_the_recorded_one(oracle, rig, blend):
    """The cast frames give gains near (1.23, 0.91, 0.91): a wrong channel sum moves the picture.  BALANCE_FLIP_SHARE, from which the
    balance bar's share of identical bytes follows, is measured here: a +-1 disturbance of 0.1 % of the covered pre-gain bytes."""
    from tests import _analytic_common as AC

    frames = AC.make_frames(3, cast=True)
    gen = AC.spec(rig, blend=blend, balance=True)
    worst = 0.0
    for s in range(3):
        pre = gen.pre_gain(*frames[s])
        k = gen.gains(*frames[s])
        share, big = AC.balance_flip_share(pre, seeds=10)
        print("%s rig, blend=%s, frame set %d: gains %s, disturbed pre-gain image: %.4f %% of the bytes change, by at most %d" % (
            rig, blend, s, np.round(k, 4), 100 * share, big))
        assert k.max() > 1.15 and big <= int(np.ceil(k.max()))
        worst = max(worst, share)
    assert worst <= AC.BALANCE_FLIP_SHARE


@pytest.mark.gpu
@pytest.mark.parametrize("blend", [False, True])
def test_hip_analytic_matches_the_specification(ffi, SB, oracle, repo_rig, blend):
    from oracle import np_analytic

    cfg = dict(oracle.DEFAULT_CFG)
    a = SB.BevGenerator.get_args()
    for k, v in cfg.items():
        setattr(a, k, v)
    frames = [repo_rig.image(n) for n in oracle.CAMERAS]
    car = np.zeros((cfg["BEV_HEIGHT"], cfg["BEV_WIDTH"], 3), np.uint8)
    car[300:700, 375:625] = 90
    bev = SB.BevGenerator(blend=blend, balance=False, rig=repo_rig.rig, projection='analytic')
    spec = np_analytic.AnalyticBevGenerator(repo_rig.rig, cfg, blend=blend)
    for c in (None, car):
        got, want = bev(*frames, c), spec(*frames, c)
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1, int(d.max())
        assert (d == 0).mean() >= 0.999, float((d == 0).mean())
    # random frames, batch call
    rnd = W.synthetic_frames(2, cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], seed=5, kind="random")
    got = bev.batch(rnd)
    for b in range(2):
        d = np.abs(got[b].astype(np.int32) - spec(*rnd[b]).astype(np.int32))
        assert d.max() <= 1 and (d == 0).mean() >= 0.999


@pytest.mark.gpu
def test_hip_analytic_with_balance_runs_and_stays_close_to_the_table_path(ffi, SB, oracle, repo_rig):
    """blend + balance through the analytic kernel on the reference's own frames: the picture stays the table path's (PSNR), an unknown
    projection is refused.  (The bar for this chain is the specification: tests/test_analytic_gpu.py, the balance tests.)"""
    cfg = dict(oracle.DEFAULT_CFG)
    a = SB.BevGenerator.get_args()
    for k, v in cfg.items():
        setattr(a, k, v)
    frames = [repo_rig.image(n) for n in oracle.CAMERAS]
    lut = SB.BevGenerator(blend=True, balance=True, rig=repo_rig.rig)(*frames)
    ana = SB.BevGenerator(blend=True, balance=True, rig=repo_rig.rig, projection='analytic')(*frames)
    assert psnr(lut, ana) > 28.0
    with pytest.raises(Exception, match="projection should be lut/analytic"):
        SB.BevGenerator(rig=repo_rig.rig, projection='exact')


@pytest.mark.gpu
@pytest.mark.parametrize("frames_per_thread", [1, 32])
def test_hip_analytic_per_pixel_kernel_f32_against_the_specification(ffi, frames_per_thread):
    """north_star's wording taken literally (bench.py: direct_stitch_analytic_perpixel_b64), without the unit plan (BEVW_ANALYTIC_UNITS=0), the
    inverse homography + fisheye model in fp32 per output pixel.  BEVW_ANALYTIC_FRAMES=1 runs k_stitch_perpixel -- one thread per pixel AND
    frame, the projection evaluated for every frame; 32 (the default amortisation) runs k_stitch_analytic on the full grid, one evaluation
    per pixel for the whole batch of 3.  Both against the fp64 specification oracle/np_analytic.py on the reference's own frames, batch of 3
    with no sprite: PSNR, share of identical bytes and the maximum difference (an fp32 arithmetic of its own: not bit for bit).  The
    switches are read once per process, hence the child."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = (
        "import numpy as np, sys\n"
        "sys.path.insert(0, %r)\n"
        "from oracle import oracle as O, np_analytic as NA\n"
        "from cameracalibration_amd.SurroundBirdEyeView import surroundBEV as SB\n"
        "from tests import _analytic_common as T, conftest as CT\n"
        "rr = CT.RepoRig()\n"
        "a = SB.BevGenerator.get_args()\n"
        "for k, v in dict(O.DEFAULT_CFG).items(): setattr(a, k, v)\n"
        "frames = [rr.image(n) for n in O.CAMERAS]\n"
        "for blend in (False, True):\n"
        "    spec = NA.AnalyticBevGenerator(rr.rig, dict(O.DEFAULT_CFG), blend=blend)(*frames)\n"
        "    bev = SB.BevGenerator(blend=blend, rig=rr.rig, projection='analytic_f32')\n"
        "    got = bev.batch(np.stack([np.stack(frames)] * 3))\n"
        "    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])\n"
        "    d = np.abs(got[0].astype(np.int32) - spec.astype(np.int32))\n"
        "    print('per-pixel fp32 kernel vs fp64 specification, blend=%%s: PSNR %%.1f dB, %%.2f %%%% identical, max %%d LSB' %% (blend, T.psnr(spec, got[0]), 100 * (d == 0).mean(), int(d.max())))\n"
        "    assert T.psnr(spec, got[0]) > 55.0 and (d == 0).mean() > 0.97 and d.max() <= 2, (T.psnr(spec, got[0]), (d == 0).mean(), d.max())\n"
        "print('per-pixel analytic ok')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BEVW_ANALYTIC_UNITS="0", BEVW_ANALYTIC_FRAMES=str(frames_per_thread)),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "per-pixel analytic ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("blend", [False, True])
def test_hip_analytic_f32_against_fp64(ffi, SB, oracle, repo_rig, blend):
    """fp32 projection (positions within ~5e-3 pixel: tests/_analytic_common.py f32_position_error) against the fp64 mode: judged by PSNR and max difference, not byte for byte"""
    cfg = dict(oracle.DEFAULT_CFG)
    a = SB.BevGenerator.get_args()
    for k, v in cfg.items():
        setattr(a, k, v)
    frames = [repo_rig.image(n) for n in oracle.CAMERAS]
    f64 = SB.BevGenerator(blend=blend, rig=repo_rig.rig, projection='analytic')(*frames)
    f32 = SB.BevGenerator(blend=blend, rig=repo_rig.rig, projection='analytic_f32')(*frames)
    d = np.abs(f64.astype(np.int32) - f32.astype(np.int32))
    print("analytic fp32 vs fp64, blend=%s: PSNR %.1f dB, %.2f %% identical, max %d LSB" % (blend, psnr(f64, f32), 100 * (d == 0).mean(), int(d.max())))
    assert psnr(f64, f32) > 55.0
    assert (d == 0).mean() > 0.97


@pytest.mark.gpu
@pytest.mark.parametrize("blend", [False, True])
def test_hip_analytic_units_on_the_bench_rig_batch_of_64(ffi, SB, oracle, blend):
    """The analytic mode on the unit schedule (wide plan: csrc/bevwarp.hip analytic_units_build, csrc/bevw_unit.h k_plan_unit_wide) on the bench
    rig with the bench's batch size, device-resident, all-random frames and a car sprite: every BEV of the batch is independent of its position
    (chunk / XCD mapping, the ragged tail of a 19-frame batch) and within 1 LSB of the fp64 specification, >= 99.9 % of the bytes identical."""
    from oracle import np_analytic

    cfg, rig = W.CONFIG_S, W.rig_s()
    a = SB.BevGenerator.get_args()
    for k, v in cfg.items():
        setattr(a, k, v)
    bw, bh = cfg["BEV_WIDTH"], cfg["BEV_HEIGHT"]
    uniq, batch = 2, 64
    frames = W.synthetic_frames(uniq, cfg["FRAME_WIDTH"], cfg["FRAME_HEIGHT"], seed=11, kind="random")
    rng = np.random.default_rng(5)
    car = np.zeros((bh, bw, 3), np.uint8)
    car[380:720, 400:680] = rng.integers(0, 256, (340, 280, 3), dtype=np.uint8)
    bev = SB.BevGenerator(blend=blend, balance=False, rig=rig, projection='analytic')
    spec = np_analytic.AnalyticBevGenerator(rig, cfg, blend=blend)
    d_in = ffi.DeviceBuffer(batch * frames[0].nbytes)
    d_car = ffi.DeviceBuffer(car.nbytes)
    d_out = ffi.DeviceBuffer(batch * bw * bh * 3)
    d_out.fill(0x5A)
    d_car.upload(car)
    for b in range(batch):
        d_in.upload(frames[b % uniq], offset=b * frames[0].nbytes)
    bev.run_device(d_in.ptr, batch, d_car.ptr, d_out.ptr)
    bev.sync()
    out = d_out.download((batch, bh, bw, 3))
    for b in range(uniq, batch):
        assert np.array_equal(out[b], out[b % uniq]), b
    for b in range(uniq):
        d = np.abs(out[b].astype(np.int32) - spec(*frames[b], car).astype(np.int32))
        assert d.max() <= 1, int(d.max())
        assert (d == 0).mean() >= 0.999, float((d == 0).mean())
    # a ragged batch through the host-buffer entry point, no sprite
    rag = bev.batch(np.concatenate([frames] * 9 + [frames[:1]]))
    want0 = spec(*frames[0])
    d = np.abs(rag[18].astype(np.int32) - want0.astype(np.int32))
    assert d.max() <= 1 and (d == 0).mean() >= 0.999
    assert np.array_equal(rag[18], rag[0]) and np.array_equal(rag[17], rag[1])
