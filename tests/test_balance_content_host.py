"""The pool of tests/_balance_content.py has teeth: conditions on the content, checked WITHOUT a GPU with the CPU oracle, in every pixel
format the GPU module runs (the NV12 / YUYV / UYVY forms are judged on their spec-converted frames: limited range and shared chroma change
the statistics of the graded sets).

1. _balance_content.Chain -- the balance chain restated from the oracle's own steps -- equals RefBevGenerator(balance=True) on every frame
   set, blend off and on.  Only then is it used for mutants.
2. Mutants, each a wrong image the GPU module must be able to see.  Delta mutants take the deltas of set b - 1, b + 1, b + 2 (modulo the
   pool), of the first set of b's slice (0 or 16), or rotate the cameras of the tuple by one; gain mutants take the gains of set b - 1,
   b + 1, b + 2.  Each must change the image of EVERY graded set.  Special sets may be insensitive, but only those EXCUSED below by name:
   sets whose deltas are all zero meet other such sets, black stays black under any gain, and sets 0 and 16 ARE the first sets of their
   slices.  The arithmetic mutants -- floor(x + 0.5) instead of round-half-even, half away from zero, the mean of
   the four sums instead of the mean of the four means -- must change at least the tie set.
3. Statistics: the delta tuples of the graded sets are pairwise distinct, finite gains span at least a factor of two over the pool, and
   every special set shows the property it is in the pool for.  The table of deltas and gains is printed (pytest -s, or the captured
   output of a failure)."""
import math

import numpy as np
import pytest

from tests import _balance_content as BC

DELTA_MUTANTS = ("deltas of b-1", "deltas of b+1", "deltas of b+2", "deltas of the slice's first set", "deltas rotated by one camera")
GAIN_MUTANTS = ("gains of b-1", "gains of b+1", "gains of b+2")
# special sets a mutant may leave unchanged, by name (what the test finds is a subset in every format; no graded set is ever excused)
EXCUSED = {
    "deltas of b-1": {"white"},            # set 0 (black) has deltas 0, as white has
    "deltas of b+1": {"black"},            # set 1 (white) has deltas 0, as black has
    "deltas of b+2": set(),
    "deltas of the slice's first set": {"black", "white", "dark"},   # sets 0 and 16 ARE the first sets; white takes black's zeros
    "deltas rotated by one camera": {"black", "white", "dark"},      # (0, 0, 0, 0) rotated
    "gains of b-1": {"black"},             # 0 times any gain, NaN included, saturates to 0
    "gains of b+1": {"black", "dark"},     # dark: bytes 0 .. 3 times the gains of set 17 (0.87 .. 1.13) round to themselves
    "gains of b+2": {"black", "white"},    # white under the gains of set 3, which are 1
}


class Analysis:
    """Deltas, pre-gain images, gains and final images of the pool in one pixel format, per blend mode."""

    def __init__(self, oracle, frames, car):
        self.frames, self.car = frames, car
        self.chain = {blend: BC.Chain(oracle, blend) for blend in (False, True)}
        self.deltas = [self.chain[False].deltas(f) for f in frames]
        self.pre = {blend: [ch.pregain(f, d) for f, d in zip(frames, self.deltas)] for blend, ch in self.chain.items()}
        self.gains = {blend: [self.chain[blend].gains(p) for p in pre] for blend, pre in self.pre.items()}
        self.image = {blend: [self.chain[blend].finish(p, g, car) for p, g in zip(self.pre[blend], self.gains[blend])] for blend in (False, True)}

    def mutant(self, name, b, blend):
        """The image of set b under mutant `name`."""
        ch, n = self.chain[blend], BC.N
        if name in GAIN_MUTANTS:
            other = (b + int(name.split("b")[1])) % n
            return ch.finish(self.pre[blend][b], self.gains[blend][other], self.car)
        if name == "deltas rotated by one camera":
            d = self.deltas[b][1:] + self.deltas[b][:1]
        elif name == "deltas of the slice's first set":
            d = self.deltas[BC.slice_first(b)]
        else:
            d = self.deltas[(b + int(name.split("b")[1])) % n]
        pre = ch.pregain(self.frames[b], d)
        return ch.finish(pre, ch.gains(pre), self.car)


_made = {}


@pytest.fixture(scope="module", params=BC.FORMATS)
def case(request, oracle):
    fmt = request.param
    frames = BC.forms(fmt)[1]
    if fmt == "uyvy":   # the byte order is a layout: the same Y, U and V reach the same texels
        assert np.array_equal(frames, BC.forms("yuyv")[1]) and not np.array_equal(BC.forms("uyvy")[0], BC.forms("yuyv")[0])
        fmt = "yuyv"
    if fmt not in _made:
        _made[fmt] = Analysis(oracle, BC.forms(fmt)[1], BC.car())
    return request.param, _made[fmt]


def test_pool_layout():
    pool = BC.bgr_pool()
    fw, fh = BC.CFG["FRAME_WIDTH"], BC.CFG["FRAME_HEIGHT"]
    assert pool.shape == (33, 4, fh, fw, 3) and pool.dtype == np.uint8
    assert sorted(BC.SPECIAL) == [0, 1, 3, 5, 7, 16, 20] and len(BC.GRADED) == 26
    assert sum(b < 9 for b in BC.SPECIAL) == 5 and sum(b < 9 for b in BC.GRADED) == 4   # batch 9 sees both kinds
    assert BC.forms("nv12")[0].shape == (33, 4, fh * 3 // 2, fw) and BC.forms("yuyv")[0].shape == (33, 4, fh, fw, 2)
    for fmt in BC.FORMATS[1:]:   # the special sets survive the conversion (2 x 2-aligned regions of round-trip colours); `dark` is random
        back = BC.forms(fmt)[1]
        assert [name for b, name in BC.SPECIAL.items() if not np.array_equal(back[b], pool[b])] == ["dark"], fmt
        assert not any(np.array_equal(back[b], pool[b]) for b in BC.GRADED), fmt
    assert np.array_equal(pool[2], BC.graded(np.random.default_rng(BC.SEED), 33, fw, fh)[2])   # deterministic


def test_chain_equals_the_oracle_generator(oracle, case):
    fmt, a = case
    for blend in (False, True):
        ref = oracle.RefBevGenerator(BC.small_rig(), BC.CFG, blend=blend, balance=True)
        for b in range(BC.N):
            assert np.array_equal(a.image[blend][b], ref(*a.frames[b], a.car)), "%s, blend %d, set %d" % (fmt, blend, b)
        assert np.array_equal(a.chain[blend].finish(a.pre[blend][2], a.gains[blend][2]), ref(*a.frames[2])), "without the car"


def test_mutants_change_every_graded_set(case):
    fmt, a = case
    print()
    for blend in (False, True):
        for name in DELTA_MUTANTS + GAIN_MUTANTS:
            same = [b for b in range(BC.N) if np.array_equal(a.mutant(name, b, blend), a.image[blend][b])]
            print("%s, blend %d, %s: insensitive sets %s" % (fmt, blend, name, [BC.SPECIAL.get(b, b) for b in same]))
            assert not [b for b in same if b in BC.GRADED], "%s, blend %d: %s leaves graded sets %s unchanged" % (fmt, blend, name, same)
            assert {BC.SPECIAL[b] for b in same} <= EXCUSED[name], "%s, blend %d: %s leaves %s unchanged" % (fmt, blend, name, same)


def test_arithmetic_mutants_change_the_tie_set(case):
    fmt, a = case
    b = BC.AT["tie"]
    ch = a.chain[True]
    raw = ch.raw_deltas(a.frames[b])
    assert raw[1:] == [-0.5, -0.5, -1.5] and 2.0 < raw[0] < 2.5, raw   # exact ties: k = -1 (odd) and k = -2 (even)
    got = {"even": a.deltas[b], "floor": ch.deltas(a.frames[b], rounding="floor"), "away": ch.deltas(a.frames[b], rounding="away"),
           "sums": ch.deltas(a.frames[b], mean="sums")}
    assert got == BC.TIE_DELTAS, (fmt, got)
    for name in ("floor", "away", "sums"):
        for blend in (False, True):
            c = a.chain[blend]
            pre = c.pregain(a.frames[b], got[name])
            assert not np.array_equal(c.finish(pre, c.gains(pre), a.car), a.image[blend][b]), "%s, blend %d: mutant '%s'" % (fmt, blend, name)
    # the graded sets hold no ties: both arithmetic mutants leave their deltas alone (the tie set is what sees them)
    assert all(ch.deltas(a.frames[g], rounding="floor") == a.deltas[g] for g in BC.GRADED)


def test_statistics_of_the_pool(oracle, case):
    fmt, a = case
    print("\n%s: set, name, deltas, gains (blend off), gains (blend on)" % fmt)
    for b in range(BC.N):
        print("%2d %-11s %-20s %s %s" % (b, BC.SPECIAL.get(b, "graded"), a.deltas[b], np.array2string(a.gains[False][b], precision=4),
                                         np.array2string(a.gains[True][b], precision=4)))
    tuples = [a.deltas[b] for b in BC.GRADED]
    assert len(set(tuples)) == len(tuples), "delta tuples of the graded sets repeat"
    assert all(any(d != 0 for d in t) for t in tuples) and max(abs(d) for t in tuples for d in t) >= 32
    at = BC.AT
    for blend in (False, True):
        g = a.gains[blend]
        finite = np.array([g[b] for b in BC.GRADED])
        assert np.isfinite(finite).all() and finite.max() / finite.min() >= 2.0, (fmt, blend, finite.min(), finite.max())
        assert np.isnan(g[at["black"]]).all()
        assert np.abs(g[at["white"]] - 1.0).max() < 1e-12   # (x + x + x) / 3 / x in fp64
        assert np.isinf(g[at["dead"]][0]) and np.isfinite(g[at["dead"]][1:]).all() and (g[at["dead"]][1:] > 0).all()
        assert 255.0 < g[at["near_dead"]][0] < np.inf and np.isfinite(g[at["near_dead"]][1:]).all()
        assert a.pre[blend][at["dead"]][..., 0].max() == 0 and a.pre[blend][at["dead"]].max(axis=-1).min(where=~BC.uncovered(a.chain[blend].plain), initial=255) > 0
    assert a.deltas[at["black"]] == a.deltas[at["white"]] == (0, 0, 0, 0)
    want = tuple(-191 if c == BC.WHITE_CAMERA else 64 for c in range(4))
    assert a.deltas[at["black_white"]] == want
    v = a.frames[at["black_white"]].max(axis=-1).astype(np.int32)   # V of a texel = max(B, G, R); the shift saturates v + delta
    shifted = v + np.array(want).reshape(4, 1, 1)
    assert (shifted > 255).any() and (shifted < 0).any(), "V saturates at both ends"
    hsv = [oracle.bgr2hsv(a.chain[False].shift(a.frames[at["black_white"]][c], want[c]))[..., 2] for c in range(4)]
    assert any((h == 255).any() for h in hsv) and any((h == 0).any() for h in hsv)
    assert a.frames[at["dark"]].max() <= 8 and a.frames[at["dark"]].max() >= 3   # bytes 0 .. 3; a YUV form adds the conversion's few LSB
    assert a.deltas[at["tie"]] == BC.TIE_DELTAS["even"]
    assert all(math.isfinite(x) for t in a.deltas for x in t)
