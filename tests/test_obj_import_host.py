"""The OBJ index rule (csrc/host/obj_import.hpp) and the host builders without a device:
csrc/tools/scene_host_check.cpp, a program of its own over the host scene pipeline, built by the
Makefile's scene_host_asan target under the address and undefined-behaviour sanitizers.  It is run
once without arguments (the builders' self-checks on synthetic boxes) and once over small OBJ
files written here: a face index that is 0, out of range, not representable or no number refuses
the file with FRT_E_INVALID, in the importer and in the tessellator; a bad texture index only
means no uv.  The same files then go through the loaded library (no sanitizer there): they raise
FrtError, and a refused add_obj leaves the scene as it was.  CPU only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import first_raytracer_amd as frt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "CornellBox-Original.obj")
OK, INVALID = 0, -1   # FRT_OK, FRT_E_INVALID

V3 = "v 0 0 0\nv 1 0 0\nv 0 1 0\n"
# name -> (text, create rc, tessellator rc, triangles)
FILES = {
    "abs": (V3 + "f 1 2 3\n", OK, OK, 1),
    "rel": (V3 + "f -3 -2 -1\n", OK, OK, 1),
    "past_end": (V3 + "f 1 2 4\n", INVALID, INVALID, 0),
    "zero": (V3 + "f 0 1 2\n", INVALID, INVALID, 0),
    "below": (V3 + "f -4 -1 -2\n", INVALID, INVALID, 0),
    "wraps": (V3 + "f 1 2 4294967297\n", INVALID, INVALID, 0),
    "huge": (V3 + "f 1 2 99999999999999999999\n", INVALID, INVALID, 0),
    "letters": (V3 + "f a b c\n", INVALID, INVALID, 0),
    "face_first": ("f 1 2 3\n" + V3, INVALID, INVALID, 0),
    "normal_past_end": (V3 + "vn 0 0 1\nf 1//1 2//1 3//2\n", INVALID, INVALID, 0),
    "quad_past_end": (V3 + "v 1 1 0\nf 1 2 3 5\n", INVALID, INVALID, 0),
    "uv_past_end": (V3 + "vt 0.5 0.5\nf 1/1 2/1 3/2\n", OK, OK, 1),
    "trailing_slashes": (V3 + "f 1/ 2// 3/\n", OK, OK, 1),   # a corner ends at white space
    "empty": ("", OK, OK, 0),
}
MALFORMED = [k for k, v in FILES.items() if v[1] == INVALID]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("obj")
    out = {}
    for name, spec in FILES.items():
        out[name] = str(d / (name + ".obj"))
        with open(out[name], "w") as f:
            f.write(spec[0])
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("asan")
    subprocess.run(["make", "-C", os.path.join(ROOT, "first_raytracer_amd"), "scene_host_asan", "OBJDIR=" + str(d)],
                   check=True, timeout=300)
    return str(d / "scene_host_asan")


def run_clean(argv):
    p = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr
    return p.stdout


def test_builders_under_sanitizers(checker):
    m = re.search(r"scene_host_check: (\d+) checks failed", run_clean([checker]))
    assert m and int(m.group(1)) == 0


def test_index_rule_under_sanitizers(checker, files, tmp_path):
    names = list(FILES)
    out = run_clean([checker, "--tess-dir", str(tmp_path)] + [files[n] for n in names] + [CORNELL])
    rec = {}
    for line in out.splitlines():
        path, _, rest = line.rpartition(": ")
        rec[path] = dict(kv.split("=") for kv in rest.split())
    for n in names:
        r, (_, create, tess, tris) = rec[files[n]], FILES[n]
        assert r["create"] == "%d/%d" % (create, create), (n, r)
        assert int(r["tess"]) == tess and int(r["n_tris"]) == tris, (n, r)
        assert int(r["sah"]) == (OK if tris else INVALID), (n, r)   # no tree over an empty world
    assert rec[files["abs"]]["geom"] == rec[files["rel"]]["geom"]   # the same vertex arrays
    assert rec[files["uv_past_end"]]["uv_zero"] == "1"
    c = rec[CORNELL]
    assert (c["create"], c["n_tris"], c["n_nodes"], c["tess"]) == ("0/0", "36", "35", "0"), c
    assert (c["sah"], c["sah_nodes"]) == ("0", "35"), c


def test_relative_indices_name_the_same_vertices(files):
    a = frt.HostScene("obj_geo", files["abs"], 1.0).arrays()
    b = frt.HostScene("obj_geo", files["rel"], 1.0).arrays()
    assert a["tri_v"].shape == (1, 9) and np.array_equal(a["tri_v"], b["tri_v"])


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_file_raises(files, name, tmp_path):
    for kind in ("cornell_box_obj", "obj_smooth", "veach_mis"):
        with pytest.raises(frt.FrtError, match="failed: invalid"):
            frt.HostScene(kind, files[name], 1.0)
    with pytest.raises(frt.FrtError, match="failed: invalid"):
        frt.write_tessellated_obj(files[name], 2, str(tmp_path / "t.obj"))


@pytest.mark.parametrize("name", MALFORMED)
def test_refused_add_obj_leaves_the_scene(files, name):
    """from_spec's sequence by hand: Cornell, then a malformed file, then the scene is finished."""
    L = frt.lib()
    ptr = ctypes.c_void_p()
    assert L.frt_scene_new(ctypes.byref(ptr)) == OK
    try:
        assert L.frt_scene_add_obj(ptr, CORNELL.encode(), None, None, 1) == OK
        before, after = frt.HostSceneInfo(), frt.HostSceneInfo()
        L.frt_scene_info(ptr, ctypes.byref(before))
        assert L.frt_scene_add_obj(ptr, files[name].encode(), None, None, 1) == INVALID
        L.frt_scene_info(ptr, ctypes.byref(after))
        counts = [n for n, _ in frt.HostSceneInfo._fields_ if n not in ("load_ms", "build_ms")]
        assert [getattr(before, n) for n in counts] == [getattr(after, n) for n in counts]
        assert (after.n_tris, after.n_materials) == (36, before.n_materials) and before.n_materials > 0
        cam = [(ctypes.c_double * 3)(*v) for v in ((0, 1, 3.9), (0, 1, 0), (0, 1, 0))]
        assert L.frt_scene_set_camera(ptr, cam[0], cam[1], cam[2], 40.0, 1.0, 0.0, 10.0) == OK
        assert L.frt_scene_finish(ptr, 0) == OK
        L.frt_scene_info(ptr, ctypes.byref(after))
        assert (after.n_tris, after.n_nodes) == (36, 35)
    finally:
        L.frt_scene_destroy(ptr)


def test_from_spec_raises_on_a_malformed_object(files):
    spec = {"objects": [{"obj": CORNELL, "geo": True}, {"obj": files["past_end"], "geo": True}],
            "camera": frt.CORNELL_CAMERA}
    with pytest.raises(frt.FrtError):
        frt.HostScene.from_spec(spec, 1.0)
