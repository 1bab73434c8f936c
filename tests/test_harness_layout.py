"""The layout of the test suite itself, on the host: shared test code lives in tests/_harness.py (and the _*.py helper of its topic) and
is imported as `tests._name`; no test module is imported by anything; the assertion helpers that moved there still refuse what they
refused (NumPy arrays only); run_child tells a failed child from a dead one (throw-away scripts that never touch the library or a GPU).

"GPU tests" below are the modules marked gpu as a whole and the _*_worker.py children.  tests/test_camera_shard.py, whose ranks start
under torch.distributed.run, and the `-c code` children that test the drop-in import layout keep their own launch."""
import ast
import glob
import os

import numpy as np
import pytest

from tests import _harness as H
from tests import _nv12_out_spec as SO

TESTS = os.path.dirname(os.path.abspath(__file__))
FILES = {os.path.basename(p): ast.parse(open(p).read()) for p in sorted(glob.glob(os.path.join(TESTS, "*.py")))}
HELPERS = {f[:-3] for f in FILES if f.startswith("_")}


def imports(tree):
    """every (module, name) a file imports, `import a.b` as ('a.b', None)"""
    for n in ast.walk(tree):
        if isinstance(n, ast.Import):
            yield from ((a.name, None) for a in n.names)
        elif isinstance(n, ast.ImportFrom):
            yield from ((n.module or "", a.name) for a in n.names)


def files_with(pred):
    return sorted(f for f, tree in FILES.items() if any(pred(n) for n in ast.walk(tree)))


def is_fixture(n, name):
    return isinstance(n, ast.FunctionDef) and n.name == name and any("fixture" in ast.unparse(d) for d in n.decorator_list)


def test_no_test_module_is_imported_and_no_helper_under_a_bare_name():
    for f, tree in FILES.items():
        for module, name in imports(tree):
            parts = module.split(".") + ([name] if name else [])
            assert not any(p.startswith("test_") for p in parts), "%s imports %s" % (f, ".".join(parts))
            assert module.split(".")[0] not in HELPERS, "%s imports helper %s under a bare name" % (f, module)


@pytest.mark.parametrize("kind,name", [("def", "small_rig"), ("def", "uncovered"), ("def", "random_car"), ("def", "assert_nv12"),
                                       ("class", "Remapper"), ("=", "SMALL_CFG")])
def test_shared_definitions_exist_once(kind, name):
    def defines(n):
        if kind == "=":
            return isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in n.targets)
        return isinstance(n, ast.ClassDef if kind == "class" else ast.FunctionDef) and n.name == name

    assert files_with(defines) == ["_harness.py"]


def test_fixtures_live_in_the_harness():
    assert files_with(lambda n: is_fixture(n, "SB")) == ["_harness.py"]
    # test_abi.py builds the library first, test_analytic_gpu.py also asserts the default switches
    assert files_with(lambda n: is_fixture(n, "ffi")) == ["_harness.py", "test_abi.py", "test_analytic_gpu.py"]


def test_gpu_tests_start_processes_through_the_harness_only():
    def whole_module_gpu(tree):
        return any(isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "pytestmark" and "mark.gpu" in ast.unparse(n.value) for n in tree.body)

    gpu = {f for f, tree in FILES.items() if whole_module_gpu(tree) or f.endswith("_worker.py")}
    assert len(gpu) > 20
    runs = set(files_with(lambda n: isinstance(n, ast.Attribute) and n.attr in ("run", "Popen", "check_output") and ast.unparse(n.value) == "subprocess"))
    assert {"_harness.py", "_native_build.py"} <= runs
    assert runs & gpu == {"test_gpu_parity.py"}, sorted(runs & gpu)   # its two `-c code` children test the drop-in import layout


# ---------------------------------------------------------------------------------------------------------------
# negative controls of the assertion helpers: 16 x 8 pixels, the left 4 columns covered by no camera
# ---------------------------------------------------------------------------------------------------------------
BH, BW = 8, 16
NONE = np.zeros((BH, BW), bool)
NONE[:, :4] = True


def image(car=False):
    img = np.random.default_rng(1).integers(1, 256, (BH, BW, 3), dtype=np.uint8)
    img[NONE] = (10, 200, 90) if car else 0
    return img


def changed(a, at, to=None):
    b = a.copy()
    b[at] = b[at] + 1 if to is None else to
    return b


def raises(f, *a, **kw):
    with pytest.raises(AssertionError):
        f(*a, **kw)


def test_assert_same_controls():
    want = image()
    H.assert_same(want.copy(), want, NONE, "equal")
    raises(H.assert_same, changed(want, (5, 9, 1)), want, NONE, "a covered byte + 1")
    raises(H.assert_same, changed(want, (2, 1, 2)), want, NONE, "a byte of a pixel no camera covers")
    raises(H.assert_same, want[:-1], want, NONE, "shape")
    raises(H.assert_equal, changed(want, (0, 0, 0)), want, "no mask")


def test_grey_assertions_controls():
    want = image()[..., 0]
    H.assert_same_gray(want.copy(), want, NONE, "equal")
    H.assert_batch_gray(np.stack([want, want]), np.stack([want, want]), NONE, "equal")
    raises(H.assert_same_gray, changed(want, (5, 9)), want, NONE, "a covered byte + 1")
    raises(H.assert_same_gray, changed(want, (2, 1)), want, NONE, "a byte outside the frame's footprint")
    raises(H.assert_same_gray, changed(want, (2, 1)), changed(want, (2, 1)), NONE, "equal, but not 0 outside")
    raises(H.assert_same_gray, want.astype(np.uint16), want, NONE, "dtype")
    raises(H.assert_batch_gray, np.stack([want, changed(want, (7, 15))]), np.stack([want, want]), NONE, "the second image")
    raises(H.assert_batch_gray, np.stack([want]), np.stack([want, want]), NONE, "batch size")


def test_assert_nv12_controls():
    want = image()
    got = SO.bgr_to_nv12(want)
    assert got.shape == (BH * 3 // 2, BW) and (got[:BH][NONE] == 16).all() and (got[BH:, :4] == 128).all()
    H.assert_nv12(got.copy(), want, NONE, "equal", black=True)
    raises(H.assert_nv12, changed(got, (5, 9)), want, NONE, "a covered Y byte + 1")
    raises(H.assert_nv12, changed(got, (2, 1)), want, NONE, "a Y byte no camera covers")
    raises(H.assert_nv12, changed(got, (BH + 1, 9)), want, NONE, "a covered U / V byte")
    raises(H.assert_nv12, changed(got, (BH + 1, 2)), want, NONE, "a U / V byte no camera covers")
    raises(H.assert_nv12, changed(got, (2, 1), 0), want, NONE, "Y 0 instead of 16", black=True)
    with pytest.raises(AssertionError, match="zeros stored instead of NV12 black"):
        H.assert_nv12(np.where(np.concatenate([NONE, NONE[::2]]), 0, got).astype(np.uint8), want, NONE, "zeros", black=False)
    car = image(car=True)   # a sprite on the pixels no camera covers: equal, and not black
    H.assert_nv12(SO.bgr_to_nv12(car), car, NONE, "car", black=False)
    with pytest.raises(AssertionError, match="NV12 black is"):
        H.assert_nv12(SO.bgr_to_nv12(car), car, NONE, "car", black=True)


@pytest.mark.parametrize("precomputed", [False, True])
@pytest.mark.parametrize("out", ["bgr", "nv12"])
def test_check_image_controls(out, precomputed):
    want = image()
    good = SO.bgr_to_nv12(want) if out == "nv12" else want
    kw = dict(want_nv12=SO.bgr_to_nv12(want)) if precomputed and out == "nv12" else {}
    H.check_image(good.copy(), want, NONE, "equal", out, black=True, **kw)
    H.check_image(good.copy(), want, NONE, "equal", out, car=None, **kw)
    raises(H.check_image, changed(good, (5, 9)), want, NONE, "a covered byte + 1", out, **kw)
    raises(H.check_image, changed(good, (2, 1)), want, NONE, "a byte no camera covers", out, **kw)
    raises(H.check_image, good[:-2], want, NONE, "shape", out, **kw)
    if out == "nv12":
        raises(H.check_image, changed(good, (BH + 1, 9)), want, NONE, "a U / V byte", out, **kw)
        raises(H.check_image, changed(good, (2, 1), 0), want, NONE, "Y 0 instead of 16", out, black=True, **kw)
        car = image(car=True)
        H.check_image(SO.bgr_to_nv12(car), car, NONE, "car", out, car=car)
        if not precomputed:   # (black is asked of an image that goes through assert_nv12)
            raises(H.check_image, SO.bgr_to_nv12(car), car, NONE, "car, but black asked", out, car=None)
    with pytest.raises(AssertionError, match="first difference at"):
        H.check_image(changed(want, (5, 9, 1)), want, NONE, "names the byte", "bgr")


# ---------------------------------------------------------------------------------------------------------------
# run_child on throw-away workers: the child only prints, sleeps or returns a number
# ---------------------------------------------------------------------------------------------------------------
def worker(tmp_path, body):
    p = tmp_path / "_layout_worker.py"
    p.write_text("import os, sys, time\n" + body + "\n")
    return str(p)


def test_run_child_passes_on_the_expected_line(tmp_path, capsys):
    p = H.run_child(worker(tmp_path, "print('worker OK', *sys.argv[1:])"), ["a", 7], expect="worker OK a 7")
    assert p.returncode == 0 and "worker OK a 7" in capsys.readouterr().out


def test_run_child_fails_the_test_on_a_plain_failure(tmp_path):
    with pytest.raises(AssertionError, match=r"worker exit 3(.|\n)*said so(.|\n)*on stderr"):
        H.run_child(worker(tmp_path, "print('said so'); print('on stderr', file=sys.stderr); sys.exit(3)"), [])
    with pytest.raises(AssertionError, match="no 'worker OK 2 cases' line"):
        H.run_child(worker(tmp_path, "print('worker OK 1 cases')"), [], expect="worker OK 2 cases")


@pytest.mark.parametrize("body,word", [("time.sleep(60)", "time limit of 1 s"), ("os._exit(139)", "status 139"), ("os._exit(134)", "status 134"),
                                       ("os._exit(124)", "status 124"), ("os._exit(137)", "status 137"), ("os.kill(os.getpid(), 15)", "status -15")])
def test_run_child_ends_the_session_on_a_dead_child(tmp_path, body, word):
    with pytest.raises(pytest.exit.Exception, match=r"_layout_worker\.py(.|\n)*" + word):
        H.run_child(worker(tmp_path, body), [], timeout=1 if "sleep" in body else 60)


def test_run_child_environment(tmp_path, monkeypatch):
    for k in ("BEVW_LAYOUT_A", "BEVW_LAYOUT_B_1", "BEVW_LAYOUT_C", "BEVW_KEPT"):
        monkeypatch.setenv(k, "parent")
    body = "print('worker OK', sorted((k, v) for k, v in os.environ.items() if k.startswith(('BEVW_LAYOUT_', 'BEVW_KEPT'))))"
    p = H.run_child(worker(tmp_path, body), [], set_env={"BEVW_LAYOUT_C": "0", "BEVW_LAYOUT_D": "5"}, drop_env=("BEVW_LAYOUT_A", "BEVW_LAYOUT_B_"))
    assert "[('BEVW_KEPT', 'parent'), ('BEVW_LAYOUT_C', '0'), ('BEVW_LAYOUT_D', '5')]" in p.stdout
