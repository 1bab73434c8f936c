"""The census of tests/_device_addresses.py -- WITHOUT a GPU: every entry-point family the GPU leg (tests/test_device_addresses_gpu.py) runs
is present with every offset it names, in every mode, every case has a name of its own, and the content is what the cases need: three frame
sets whose luminance deltas differ (so that a balance step that reads the deltas of another set shows), and a car sprite that is not
empty.  This keeps a family from passing emptily after a refactor of the catalogue; what the kernels make of the cases is the GPU leg's."""
import numpy as np
import pytest

from tests import _balance_content as BC
from tests import _device_addresses as DA

HANDLES = DA.stitch_handles()


@pytest.mark.parametrize("family", sorted(DA.REQUIRED))
def test_every_stitch_family_holds_every_offset_in_every_mode(family):
    for mode in DA.MODES:
        hs = [h for h in HANDLES if h.family == family and h.mode == mode]
        inputs = DA.FAMILY_INPUTS.get(family)
        assert len(hs) == 1 if inputs is None else sorted(h.inp for h in hs) == sorted(inputs), (family, mode)
        for h in hs:
            single = {next(iter(DA.moved(s))) for s in h.steps if len(DA.moved(s)) == 1}
            assert DA.REQUIRED[family] <= single, "%s: no step of its own for %s" % (h.name, sorted(DA.REQUIRED[family] - single))
            # the aligned control comes first and last, and expects what the handle's schedule gives an aligned step
            control = DA.PER_PIXEL if h.schedule == "per_pixel" else DA.UNITS
            assert not DA.moved(h.steps[0]) and not DA.moved(h.steps[-1]) and h.steps[0].expect == h.steps[-1].expect == control, h.name
            for s in h.steps:
                odd = any(off % 4 for _, off in DA.moved(s))
                want = DA.REFUSE if (odd and h.pitch == "aligned") else DA.PER_PIXEL if (odd or h.schedule == "per_pixel") else DA.UNITS
                assert s.expect == want, s.name


def test_what_only_some_families_have():
    by = lambda family: [h for h in HANDLES if h.family == family]
    assert len(HANDLES) == 3 * 10 and {h.mode for h in HANDLES} == set(DA.MODES)
    assert all(any(len(DA.moved(s)) == 2 for s in h.steps) for h in by("nv12_out")), "car and out at once"
    assert all(h.out == "nv12" for h in by("nv12_out")) and all(h.out == "bgr" for h in HANDLES if h.family != "nv12_out")
    assert all(not h.with_car and not any(s.car for s in h.steps) for h in by("no_car")) and all(h.with_car for h in HANDLES if h.family != "no_car")
    assert all(h.cfg == "bw250" for h in by("padded_scratch")) and DA.CFGS["bw250"]["BEV_WIDTH"] == 250 and DA.CFGS["small"]["BEV_WIDTH"] == 248
    assert all(h.surfaces and not any(s.frames for s in h.steps) for h in by("surfaces")), "the planes stay aligned, as the contract demands"
    assert all(h.pitch == "aligned" and sum(s.expect == DA.REFUSE for s in h.steps) == 3 for h in by("pitched"))
    assert all(h.pitch == "dense" and not any(s.expect == DA.REFUSE for s in h.steps) for h in HANDLES if h.family != "pitched")
    # the 16-byte gate of the 4:2:2 V sums: frames at +4, +8, +12 stay on the units
    for h in by("formats_in"):
        assert {s.frames for s in h.steps if s.expect == DA.UNITS} == {0, 4, 8, 12}, h.name


def test_remapper_matrix():
    hs = DA.remap_handles()
    assert sorted((h.maps, h.inp, h.out) for h in hs) == sorted((m, i, o) for m in DA.REMAP_MAPS for i in DA.REMAP_INPUTS for o in DA.REMAP_OUTPUTS)
    assert DA.REMAP_INPUTS == ("bgr", "nv12", "yuyv") and DA.REMAP_OUTPUTS == ("bgr", "nv12") and len(DA.REMAP_MAPS) == 2
    for h in hs:
        assert {(s.src, s.dst) for s in h.steps if s.expect == DA.PER_PIXEL} == {(o, 0) for o in DA.ODD} | {(0, o) for o in DA.ODD}, h.name
        assert {(s.src, s.dst) for s in h.steps if s.expect == DA.UNITS} == {(0, 0), (4, 0), (12, 0)}, h.name
        assert (h.steps[0].src, h.steps[0].dst) == (h.steps[-1].src, h.steps[-1].dst) == (0, 0)


def test_jpeg_cases():
    assert DA.JPEG_SIZES == ((40, 56), (17, 33), (100, 75)) and DA.JPEG_FILES == 3 and [s for s, _ in DA.JPEG_SUBSAMPLINGS] == ["420", "444"]
    for h, w in DA.JPEG_SIZES:
        dec = DA.decode_cases(h, w, "420")
        assert {(c.off, c.pitch - w * 3, c.stride - c.pitch * h) for c in dec} == {(o, p, s) for o in (0, 1, 2, 3) for p in (0, 1, 4, 7) for s in (0, 5)}
        enc = DA.encode_cases(h, w)
        assert {(c.off, c.pitch - w * 3) for c in enc} == {(o, p) for o in (1, 2, 3) for p in (1, 4)}
        assert all(c.stride >= c.pitch * h and c.pitch >= w * 3 for c in dec + enc)
        ims = DA.jpeg_images(h, w)
        assert ims.shape == (3, h, w, 3) and len({im.tobytes() for im in ims}) == 3
    assert DA.ENCODE_PADDING == 77


def test_every_case_name_is_unique():
    names = DA.all_names()
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)[:5]
    assert len(names) == 216 + 120 + 192 + 36, len(names)   # stitch steps, remapper steps, decodes, encodes


def test_arena_offsets_fit_the_slack():
    offs = [getattr(s, w) for h in HANDLES for s in h.steps for w in ("frames", "car", "out")] + [o for h in DA.remap_handles() for s in h.steps for o in (s.src, s.dst)]
    assert 0 <= min(offs) and max(offs) == 12 < DA.SLACK and DA.SLACK % 16 == 0 and DA.FILL == 0x5A


@pytest.mark.parametrize("fmt", BC.FORMATS)
def test_the_three_frame_sets_have_distinct_luminance_deltas(oracle, fmt):
    """per pixel format: the deltas are those of the frames the input specification makes of what the engine is given"""
    native, back = DA.content(fmt)
    assert native.shape[:2] == back.shape[:2] == (DA.BATCH, 4) == (3, 4) and back.shape[2:] == (256, 320, 3)
    chain = BC.Chain(oracle, blend=False)
    deltas = [chain.deltas(back[b]) for b in range(DA.BATCH)]
    print(fmt, deltas)
    assert len(set(deltas)) == DA.BATCH, deltas
    assert all(len(set(d)) >= 3 and max(abs(x) for x in d) >= 4 for d in deltas), "a set whose cameras hardly differ: %s" % (deltas,)


@pytest.mark.parametrize("cfg", sorted(DA.CFGS))
def test_the_car_is_not_empty(cfg):
    car = DA.car(cfg)
    c = DA.CFGS[cfg]
    assert car.shape == (c["BEV_HEIGHT"], c["BEV_WIDTH"], 3) and np.count_nonzero(car.any(-1)) >= 0.9 * c["CAR_WIDTH"] * c["CAR_HEIGHT"]
    assert len(np.unique(car)) == 256
