"""The launch plans, pinned: which kernel instantiation, with how much LDS, every
(scene, call) of a grid gets -- frtx_selftest_plan runs the library's dispatch
(pick_launcher, pick_mlt, pick_trace) over a context built on the host -- against
the recorded table tests/golden/plans.json.  The grid sits on both sides of every
boundary of the residency rule and the stack classes, and every kernel a render
or a ray query can reach occurs in the table.  CPU only.

  python tests/test_plans_host.py --record     rewrites the table from the built library

The table: "kernels" = the distinct kernel names, "answers" = the distinct
answers as integer rows (ANSWER's order; kernels by index, -1 = none), "rows" =
one answer index per grid row, "grid_sha256" = the hash of the grid's queries."""
import hashlib
import itertools
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import first_raytracer_amd as frt  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "plans.json")
ANSWER = ("rc", "kernel", "kernel_boot", "lds", "stack", "waves", "lds_scene", "wide", "f64", "scene_lds", "lds_boot")
QUERY = tuple(n for n, _ in frt.PlanQuery._fields_)

BVH, LIST = frt.FRT_WORLD_BVH, frt.FRT_WORLD_LIST
PATH, MLT, AO, NORMALS = (frt.FRT_INTEGRATOR_PATH, frt.FRT_INTEGRATOR_PSSMLT, frt.FRT_INTEGRATOR_AO,
                          frt.FRT_INTEGRATOR_NORMALS)
ALBEDO, DEPTH = frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH
ROULETTE, SOBOL, NEE = frt.FRT_FLAG_ROULETTE, frt.FRT_FLAG_SOBOL, frt.FRT_FLAG_ENV_SAMPLING
AUTO, FP32, FP64 = frt.FRT_PRECISION_AUTO, frt.FRT_PRECISION_FP32, frt.FRT_PRECISION_FP64
# the material sets (csrc/frt_path.hpp kMats*): none, textures, specular, both, every material
MATS = (0, 1, 2, 3, 7)
# every subset of the estimator flags, then the A/B flags one at a time
ESTIMATORS = tuple(sum(s) for n in range(4) for s in itertools.combinations((ROULETTE, SOBOL, NEE), n))
AB = (frt.FRT_FLAG_NO_LDS_SCENE, frt.FRT_FLAG_NO_OCT, frt.FRT_FLAG_BVH2, frt.FRT_FLAG_WAVES4, frt.FRT_FLAG_WAVES5,
      frt.FRT_FLAG_WAVES6)
# (precision, has_f64, flag): the context's setting with and without fp64 records, and the per-call overrides
PRECISIONS = ((AUTO, 0, 0), (AUTO, 1, 0), (FP32, 1, 0), (FP64, 0, 0), (FP64, 1, 0), (AUTO, 1, frt.FRT_FLAG_FP64),
              (AUTO, 0, frt.FRT_FLAG_FP64), (FP64, 1, frt.FRT_FLAG_FP32))
# scene bytes (planar, octant copies) around kLdsSceneBytes = 16 KiB and kLdsOctBytes = 14 KiB:
# the octant copies fit; the planar tree only; neither
BYTES = ((4096, 14336), (16384, 14337), (16385, 40000))
# the 4-wide tree: none; its stack fits (3 * 18 <= 12 + 44); it does not (3 * 19 > 56)
WIDE = ((0, 0), (1, 18), (1, 19))
STACKS = (7, 8, 15, 16, 23, 24, 31, 32, 63, 64)


def scene(world, stack=0, nbytes=(0, 0), wide=(0, 0)):
    return dict(world_kind=world, stack_needed=stack, scene_lds_bytes=nbytes[0], scene_lds_bytes_oct=nbytes[1],
                has_bvh4=wide[0], depth4=wide[1])


SCENES = [scene(LIST)] + [scene(BVH, d, b, w) for d in STACKS for b in BYTES for w in WIDE]
# the precision rows: the stack classes of the fp64 kernels, LDS-resident and not, with and without the wide tree
SCENES_F64 = [scene(LIST)] + [scene(BVH, d, b, w) for d in (15, 16, 31, 32, 63, 64) for b in (BYTES[0], BYTES[2])
                              for w in WIDE[:2]]


def grid():
    """The queries, in the table's order: (environment, PlanQuery fields)."""
    rows = []

    def add(s, env=None, **call):
        q = dict.fromkeys(QUERY, 0)
        q.update(s)
        q.update(call)
        q["has_spec_mats"] = int(q["mats"] != 0)
        rows.append((env or {}, q))

    def sampling(image, flags):
        """env_sampling of a path render: the image's tables exist, or (a dark image) do not"""
        return (1, 0) if image and (flags & NEE) else (0,)

    # path: every scene, material set and flag, with and without an image (AUTO: a list world renders in fp64)
    for s, m, image, f in itertools.product(SCENES, MATS, (0, 1), ESTIMATORS + AB):
        for es in sampling(image, f):
            add(s, integrator=PATH, flags=f, mats=m, env_image=image, env_sampling=es, has_f64=1)
    # path: the precisions
    for (prec, has, pf), s, m, image, f in itertools.product(PRECISIONS, SCENES_F64, MATS, (0, 1), ESTIMATORS):
        add(s, integrator=PATH, flags=f | pf, mats=m, env_image=image, env_sampling=sampling(image, f)[0], has_f64=has,
            precision=prec)
    # AO, normals, albedo, depth: one kernel set each whatever the scene's materials and the estimator flags
    for kind, s, m, image, f in itertools.product((AO, NORMALS, ALBEDO, DEPTH), SCENES, (0, 7), (0, 1),
                                                  (0, ROULETTE | SOBOL | NEE) + AB):
        add(s, integrator=kind, flags=f, mats=m, env_image=image)
    for kind, (prec, has, pf) in itertools.product((AO, NORMALS, ALBEDO, DEPTH), PRECISIONS):   # ... and the precision
        add(SCENES[0], integrator=kind, flags=pf, has_f64=has, precision=prec)
    # PSS-MLT (render_impl refuses the estimator flags before the plan)
    for s, m, image, f in itertools.product(SCENES, (0, 7), (0, 1), (0,) + AB):
        add(s, integrator=MLT, flags=f, mats=m, env_image=image)
    # ray queries
    for s, f in itertools.product(SCENES, (0,) + AB):
        add(s, kind=1, flags=f)
    for w, s, f in itertools.product(("6", "8", "10", "7"), SCENES, (0, frt.FRT_FLAG_NO_LDS_SCENE)):
        add(s, {"FRT_TRACE_WAVES": w}, kind=1, flags=f)
    # FRT_MATS_WAVES: the register cap of the tunable plans' material kernels (and of no other kernel)
    for w, s, m, image, f in itertools.product(("3", "4", "5", "6", "0"), SCENES, MATS, (0, 1),
                                               (0, frt.FRT_FLAG_NO_LDS_SCENE, frt.FRT_FLAG_WAVES5, ROULETTE)):
        add(s, {"FRT_MATS_WAVES": w}, integrator=PATH, flags=f, mats=m, env_image=image, has_f64=1)
    return rows


def grid_hash(rows):
    return hashlib.sha256(json.dumps(rows, sort_keys=True).encode()).hexdigest()


def answers(rows):
    """The library's answer to every query: ANSWER-ordered tuples, the kernels by name."""
    saved = {k: os.environ.pop(k, None) for k in ("FRT_MATS_WAVES", "FRT_TRACE_WAVES")}
    try:
        out = []
        for env, q in rows:
            os.environ.update(env)
            a = frt.selftest_plan(**q)
            for k in env:
                del os.environ[k]
            # a plan without a name for its kernel is an error of the table, never a row of it
            assert a["rc"] != 0 or a["kernel"], ("no kernel name", env, q, a)
            assert q["integrator"] != MLT or q["kind"] or a["rc"] != 0 or a["kernel_boot"], ("no kernel name", q, a)
            out.append(tuple(a[k] for k in ANSWER))
        return out
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def record():
    rows = grid()
    got = answers(rows)
    kernels = sorted({a[k] for a in got for k in (1, 2) if a[k]})
    number = {name: i for i, name in enumerate(kernels)}
    packed = [tuple(number.get(v, -1) if k in (1, 2) else v for k, v in enumerate(a)) for a in got]
    distinct = sorted(set(packed))
    index = {a: i for i, a in enumerate(distinct)}
    with open(TABLE, "w") as f:
        json.dump({"grid_sha256": grid_hash(rows), "kernels": kernels, "answers": distinct,
                   "rows": [index[a] for a in packed]}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(rows)} rows, {len(distinct)} distinct answers, {len(kernels)} kernels -> {TABLE}")


def table():
    with open(TABLE) as f:
        return json.load(f)


def test_every_plan_is_the_recorded_one():
    t = table()
    rows = grid()
    assert grid_hash(rows) == t["grid_sha256"] and len(rows) == len(t["rows"]), "the grid is not the recorded one"
    names = t["kernels"] + [None]
    want = [tuple(names[v] if k in (1, 2) else v for k, v in enumerate(t["answers"][i])) for i in t["rows"]]
    got = answers(rows)
    bad = [(env, q, dict(zip(ANSWER, w)), dict(zip(ANSWER, g))) for (env, q), w, g in zip(rows, want, got) if w != g]
    assert not bad, (len(bad), bad[:3])


def test_the_grid_sits_on_every_boundary():
    """Both outcomes of every rule of the dispatch occur: each return code, each residency, each stack class."""
    t = table()
    a = [dict(zip(ANSWER, t["answers"][i])) for i in set(t["rows"])]
    assert {x["rc"] for x in a} == {0, -1, -4}        # ok; fp64 without fp64 records; deeper than 63 levels
    ok = [x for x in a if x["rc"] == 0]
    assert {x["stack"] for x in ok} == {0, 8, 12, 16, 24, 32, 64}
    assert {x["waves"] for x in ok} == {0, 1, 3, 4, 5, 6, 7, 8, 10}
    # in LDS: the octant copies of the first class, the planar tree of the first two
    assert {x["scene_lds"] for x in ok} == {0, BYTES[0][1], BYTES[0][0], BYTES[1][0]}
    assert {(x["lds_scene"], x["wide"], x["f64"]) for x in ok} == {(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)}


# kernels no plan chooses: the film reductions, the denoiser, the error film, the multi-GPU film
# kernels and the BVH builders (their own and rocprim's sort kernels)
NOT_PLANNED = ("film_reduce", "film_reduce_mean", "mlt_film_to_float", "denoise_deslot", "denoise_reslot",
               "denoise_filter", "film_error", "scatter_shards", "film_add", "k_centroid_bounds", "k_morton",
               "k_hierarchy", "k_refit", "k_ploc_init", "k_ploc_nn", "k_ploc_flags", "k_ploc_merge", "k_sah_level", "rocprim")


def test_every_kernel_of_the_library_is_in_the_table():
    in_library = set(frt.kernel_handles().values())
    assert len(in_library) > 800, len(in_library)
    out = subprocess.run(["c++filt"], input="\n".join(sorted(in_library)), capture_output=True, text=True, check=True)
    plain = dict(zip(sorted(in_library), out.stdout.splitlines()))
    base = lambda n: re.match(r"(?:void )?(?:\(anonymous namespace\)::|frt::)*(\w+)", plain[n]).group(1)   # noqa: E731
    planned = {n for n in in_library if base(n) not in NOT_PLANNED}
    assert {base(n) for n in planned} == {"path_megakernel", "trace_kernel", "mlt_bootstrap", "mlt_megakernel"}
    missing = planned - set(table()["kernels"])
    assert not missing, (len(missing), sorted(plain[n] for n in missing)[:20])
    assert set(table()["kernels"]) <= in_library


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    record()
