"""first_raytracer_amd -- MI355X-native path-tracing integrator (drop-in for
jammm/first_raytracer's path::Li / path::Render hot path).

The product is native: libfrt.so (HIP kernels for gfx950 + the C++ host scene
pipeline) behind the C-ABI in include/frt.h.  This module is a thin ctypes
binding used by the tests, bench.py and scripts; it never falls back to a CPU
path -- if libfrt.so is missing or no gfx950 device is present, it raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# FRT_LIB_PATH: an experiment build (Makefile `exp` target) for timing A/B only
LIB_PATH = os.environ.get("FRT_LIB_PATH") or os.path.join(HERE, "libfrt.so")

FRT_WORLD_BVH, FRT_WORLD_LIST = 0, 1
FRT_MAT_LAMBERTIAN, FRT_MAT_DIFFUSE_LIGHT = 0, 1
FRT_PRIM_SPHERE = 1 << 30
ABI_VERSION = 9                 # include/frt.h FRT_ABI_VERSION (frt_stats / frt_material layout)
FRT_MAT_LAMBERTIAN, FRT_MAT_DIFFUSE_LIGHT, FRT_MAT_MODIFIED_PHONG, FRT_MAT_METAL, FRT_MAT_DIELECTRIC = 0, 1, 2, 3, 4
FRT_MAT_ROUGH_CONDUCTOR = 5
FRT_DIST_GGX, FRT_DIST_BECKMANN = 0, 1
FRT_TEX_CONSTANT, FRT_TEX_CHECKER, FRT_TEX_IMAGE = 0, 1, 2
FRT_IMAGE_SRGB8, FRT_IMAGE_F32 = 0, 1
FRT_FLAG_NO_LDS_SCENE = 1
FRT_FLAG_WAVES5 = 2
FRT_FLAG_WAVES6 = 4
FRT_FLAG_WAVES4 = 8
FRT_FLAG_BVH2 = 16
FRT_FLAG_NO_OCT = 256
FRT_FLAG_FP64 = 512
FRT_FLAG_FP32 = 1024
FRT_FLAG_ENV_SAMPLING = 2048   # path: next-event estimation toward the environment image (frt.h)
FRT_FLAG_ROULETTE = 4096       # path: Russian roulette from the fourth vertex on (frt.h)
FRT_FLAG_SOBOL = 8192          # path: Owen-scrambled Sobol' sample points (frt.h)
FRTX_PRT_UNSHADOWED = 1 << 16  # prt_transfer: bounce 0 without visibility rays (frt.h)
PRT_COEFFS = 25                # 5 SH bands, index l (l + 1) + m
FRT_PRECISION_AUTO, FRT_PRECISION_FP32, FRT_PRECISION_FP64 = 0, 1, 2
FRT_GPU_BVH_PLOC = 0
FRT_GPU_BVH_LBVH = 1
FRT_GPU_BVH_SAH = 2
FRT_INTEGRATOR_PATH, FRT_INTEGRATOR_PSSMLT, FRT_INTEGRATOR_AO, FRT_INTEGRATOR_NORMALS = 0, 1, 2, 3
# first-hit feature images and the feature-guided film filter (frt.h; not in the reference)
FRT_INTEGRATOR_ALBEDO, FRT_INTEGRATOR_DEPTH, FRT_INTEGRATOR_DENOISE = 4, 5, 6
FRT_INTEGRATOR_ERROR = 8        # variance film of the context's last render (frt.h; 7 is not assigned)

ERRORS = {0: "ok", -1: "invalid", -2: "hip", -3: "no scene", -4: "unsupported", -5: "io", -6: "no gfx950 device"}


class FrtError(RuntimeError):
    pass


class Material(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("distribution", ctypes.c_int32),
                ("albedo", ctypes.c_double * 3), ("emit", ctypes.c_double * 3),
                ("specular", ctypes.c_double * 3), ("exponent", ctypes.c_double), ("ior", ctypes.c_double),
                ("alpha", ctypes.c_double), ("eta", ctypes.c_double * 3), ("k", ctypes.c_double * 3),
                ("texture", ctypes.c_int32), ("image", ctypes.c_int32), ("tex_odd", ctypes.c_double * 3),
                ("tex_scale", ctypes.c_double * 2)]

    @classmethod
    def from_spec(cls, m):
        """frt_material from a scene-spec material dict (see HostScene.from_spec)."""
        r = cls()
        r.type = MAT_TYPES[m["type"]]
        r.distribution = DISTRIBUTIONS[m.get("distribution", "ggx").lower()]
        for k in ("albedo", "emit", "specular", "eta", "k"):
            getattr(r, k)[:] = [float(x) for x in m.get(k, (0.0, 0.0, 0.0))]
        r.exponent = float(m.get("exponent", 0.0))
        r.ior = float(m.get("ior", 0.0))
        r.alpha = float(m.get("alpha", 0.0))
        tex = m.get("checker")               # {"odd": rgb, "scale": (u_scale, v_scale)}
        if tex is not None:
            r.texture = FRT_TEX_CHECKER
            r.tex_odd[:] = [float(x) for x in tex["odd"]]
            r.tex_scale[:] = [float(x) for x in tex["scale"]]
        if m.get("image") is not None:       # index into the spec's "images"
            r.texture = FRT_TEX_IMAGE
            r.image = int(m["image"])
        return r


class Image(ctypes.Structure):
    """frt_image: a decoded image for FRT_TEX_IMAGE (image_texture, texture.h:51-95)."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("format", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("data", ctypes.c_void_p)]


def image_array(img):
    """(contiguous texel array, FRT_IMAGE_* format) of a spec image
    {"data": (ny, nx, 3) uint8 (sRGB, stb's LDR bytes) or float32 (HDR)}."""
    a = np.asarray(img["data"])
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("image data must be (ny, nx, 3)")
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a), FRT_IMAGE_SRGB8
    return np.ascontiguousarray(a, np.float32), FRT_IMAGE_F32


# cornell_box_obj's camera (main.cpp:236-242): lookfrom (0, 1, 3.9f), vfov 40, focus 10
CORNELL_CAMERA = {"lookfrom": (0.0, 1.0, float(np.float32(3.9))), "lookat": (0.0, 1.0, 0.0), "vup": (0.0, 1.0, 0.0),
                  "vfov": 40.0, "aperture": 0.0, "focus": 10.0}
MAT_TYPES = {"lambertian": 0, "diffuse_light": 1, "modified_phong": 2, "metal": 3, "dielectric": 4,
             "rough_conductor": 5}                      # FRT_MAT_*
DISTRIBUTIONS = {"ggx": 0, "beckmann": 1}               # FRT_DIST_*
SPHERE_WHERE = {"world": 1, "lights": 2, "both": 3}     # FRT_SPHERE_*


class SceneView(ctypes.Structure):
    _fields_ = [
        ("world_kind", ctypes.c_int32),
        ("n_tris", ctypes.c_int32),
        ("tri_v", ctypes.c_void_p), ("tri_n", ctypes.c_void_p), ("tri_material", ctypes.c_void_p),
        ("tri_geometry_normal", ctypes.c_void_p), ("tri_inv_area", ctypes.c_void_p),
        ("n_spheres", ctypes.c_int32), ("sphere", ctypes.c_void_p), ("sphere_material", ctypes.c_void_p),
        ("n_materials", ctypes.c_int32), ("materials", ctypes.c_void_p),
        ("n_nodes", ctypes.c_int32), ("root", ctypes.c_int32),
        ("node_box", ctypes.c_void_p), ("node_child", ctypes.c_void_p),
        ("n_list", ctypes.c_int32), ("list", ctypes.c_void_p),
        ("n_lights", ctypes.c_int32), ("lights", ctypes.c_void_p),
        ("cam_origin", ctypes.c_double * 3), ("cam_lower_left", ctypes.c_double * 3),
        ("cam_horizontal", ctypes.c_double * 3), ("cam_vertical", ctypes.c_double * 3),
        ("cam_u", ctypes.c_double * 3), ("cam_v", ctypes.c_double * 3),
        ("cam_lens_radius", ctypes.c_double),
        ("env_color", ctypes.c_double * 3),
        ("cam_w", ctypes.c_double * 3),
        ("cam_half_height", ctypes.c_double),
        ("tri_uv", ctypes.c_void_p),
        ("n_images", ctypes.c_int32), ("images", ctypes.c_void_p),
    ]


class RenderParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("nx", "ny", "spp")] + [("seed", ctypes.c_uint32)] + [
        (n, ctypes.c_int32) for n in ("max_depth", "integrator", "tile_size", "shard_index", "shard_count",
                                      "samples_per_item", "flags", "mlt_chains", "mlt_bootstrap", "sample_offset")]

    @classmethod
    def make(cls, nx, ny, spp, seed=0, max_depth=33, tile_size=32, shard_index=0, shard_count=1,
             samples_per_item=0, flags=0, integrator=0, sample_offset=0):
        """integrator: FRT_INTEGRATOR_PATH (path.cpp), _AO (ao.cpp), _NORMALS (debug_renderer.h),
        _ALBEDO / _DEPTH (first-hit feature images), _DENOISE (Context.denoise) or _ERROR
        (Context.render_error);
        sample_offset: first global sample index (progressive passes)."""
        return cls(nx=nx, ny=ny, spp=spp, seed=seed, max_depth=max_depth, integrator=integrator, tile_size=tile_size,
                   shard_index=shard_index, shard_count=shard_count, samples_per_item=samples_per_item, flags=flags,
                   mlt_chains=0, mlt_bootstrap=0, sample_offset=sample_offset)

    @classmethod
    def pssmlt(cls, nx, ny, mutations_per_pixel, chains, seed=0, bootstrap=10000, shard_index=0, shard_count=1,
               flags=0):
        """PSS-MLT (pssmlt.cpp): total mutations = mutations_per_pixel*nx*ny over `chains` chains."""
        return cls(nx=nx, ny=ny, spp=mutations_per_pixel, seed=seed, max_depth=10, integrator=FRT_INTEGRATOR_PSSMLT,
                   tile_size=32, shard_index=shard_index, shard_count=shard_count, samples_per_item=0, flags=flags,
                   mlt_chains=chains, mlt_bootstrap=bootstrap)


class Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("camera_rays", "extension_rays", "shadow_rays", "samples",
                                               "pixels", "work_items")] + [
        ("kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double)] + [
        (n, ctypes.c_uint32) for n in ("scene_in_lds", "waves_cap", "stack_entries", "bvh_depth")] + [
        ("scene_bytes", ctypes.c_uint64), ("fp64", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    @property
    def rays(self):
        return self.camera_rays + self.extension_rays + self.shadow_rays

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["rays"] = self.rays
        return d


class TreeCost(ctypes.Structure):
    """frt_tree_cost: a binary tree priced on the refinement pass's validation rays."""
    _fields_ = [("v", ctypes.c_double), ("t", ctypes.c_double), ("j", ctypes.c_double), ("w", ctypes.c_double),
                ("depth", ctypes.c_int32), ("n_nodes", ctypes.c_int32), ("n_rays", ctypes.c_int32),
                ("applies", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShadowTreeInfo(ctypes.Structure):
    """frt_shadow_tree_info: what the shadow-tree pass dropped and built, and what it saves."""
    _fields_ = [(n, ctypes.c_int32) for n in ("why", "kept_prims", "dropped_prims", "rule_a", "rule_b", "nodes_main",
                                              "nodes_added", "nodes_shared", "root", "empty", "n_rays",
                                              "root_stops_main", "root_stops_shadow", "n_nodes")] + [
        (n, ctypes.c_double) for n in ("v_main", "t_main", "v_shadow", "t_shadow")] + [
        ("segments", ctypes.c_int64), ("segment_hits", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ExitTreeInfo(ctypes.Structure):
    """frt_exit_tree_info: what the exit-tree pass took, and what it saves."""
    _fields_ = [(n, ctypes.c_int32) for n in ("why", "classes", "taken", "budget_refused", "nodes_off", "n_nodes",
                                              "nodes_added", "depth_off", "depth_on", "n_rays", "n_ext", "reserved")] + [
        (n, ctypes.c_int64) for n in ("lds_bytes", "lds_bytes_oct", "lds_cap", "lds_cap_oct")] + [
        (n, ctypes.c_double * 2) for n in ("v_all", "t_all", "j_all", "v_ext", "t_ext")]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if t is ctypes.c_double * 2 else getattr(self, k)) for k, t in self._fields_}


class PlanQuery(ctypes.Structure):
    """frt_plan_query: the scene properties and the call whose launch plan selftest_plan asks for."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "integrator", "flags", "world_kind", "stack_needed", "has_bvh4",
                                              "depth4", "mats", "has_spec_mats", "env_image", "env_sampling",
                                              "has_f64", "precision")] + [
        ("scene_lds_bytes", ctypes.c_int64), ("scene_lds_bytes_oct", ctypes.c_int64)]


class PlanAnswer(ctypes.Structure):
    """frt_plan_answer: the dispatch's return code, the plan's fields and the kernel handles' offsets."""
    _fields_ = [(n, ctypes.c_int32) for n in ("rc", "stack", "waves", "lds_scene", "wide", "f64")] + [
        (n, ctypes.c_int64) for n in ("lds", "scene_lds", "lds_boot")] + [
        ("kernel", ctypes.c_uint64), ("kernel_boot", ctypes.c_uint64)]


class HostSceneInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_tris", "n_spheres", "n_materials", "n_lights", "n_nodes",
                                              "world_kind", "n_list", "bvh_depth")] + [
        ("load_ms", ctypes.c_double), ("build_ms", ctypes.c_double)]


_lib = None

# every symbol include/frt.h declares
EXPORTS = ("frt_get_abi_version", "frt_create", "frt_destroy", "frt_last_error", "frt_set_precision", "frt_upload_scene",
           "frt_shard_slot_count", "frt_shard_slots", "frt_render", "frt_render_multi", "frt_render_device", "frt_trace_device",
           "frt_mlt_chain_state",
           "frt_scene_create", "frt_scene_new", "frt_scene_add_obj", "frt_scene_add_sphere", "frt_scene_set_camera",
           "frt_scene_set_env", "frt_scene_add_image", "frt_scene_finish", "frt_scene_build_bvh_gpu",
           "frt_scene_build_bvh_sah", "frt_scene_build_bvh_gpu_algo",
           "frt_scene_view_get", "frt_scene_info", "frt_scene_destroy", "frt_write_tessellated_obj",
           "frt_write_pfm", "frt_film_accumulate", "frt_tonemap_u8", "frt_write_image", "frt_selftest_path_host",
           "frt_selftest_mlt_paths_host",
           "frt_set_env_image", "frt_scene_set_env_image", "frt_scene_env_image", "frt_read_hdr",
           "frt_selftest_path_host_env")
# further self-test hooks (frt.h "frtx_*"): beside the frt_* entry points, not among them
EXPORTS_X = ("frtx_selftest_tree_refine", "frtx_selftest_trace_host", "frtx_selftest_chunk_variance",
             "frtx_selftest_plan", "frtx_selftest_shadow_tree", "frtx_render_pixels", "frtx_render_pixels_device",
             "frtx_selftest_exit_tree", "frtx_radiance_rays", "frtx_radiance_rays_device", "frtx_camera_rays_device",
             "frtx_selftest_radiance_host", "frtx_selftest_camera_rays_host",
             "frtx_prt_basis", "frtx_sh_project_image", "frtx_prt_sample_dirs", "frtx_prt_corners", "frtx_prt_transfer",
             "frtx_prt_transfer_device", "frtx_prt_rays", "frtx_prt_rays_device", "frtx_selftest_prt_transfer_host",
             "frtx_selftest_prt_rays_host", "frtx_prt_render", "frtx_selftest_prt_budget")


def lib():
    """Load libfrt.so (built in-tree by __graft_entry__.build()).  Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FrtError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 (same
    # soname as /opt/rocm's).  Load torch first so libfrt.so binds to that
    # copy; loading libfrt first would bind torch to the other runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    L.frt_get_abi_version.restype = ctypes.c_int
    if L.frt_get_abi_version() != ABI_VERSION:
        raise FrtError(f"{LIB_PATH}: ABI version {L.frt_get_abi_version()}, binding expects {ABI_VERSION}; rebuild")
    L.frt_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.frt_destroy.argtypes = [vp]
    L.frt_last_error.argtypes = [vp]
    L.frt_last_error.restype = ctypes.c_char_p
    L.frt_set_precision.argtypes = [vp, ctypes.c_int]
    L.frt_upload_scene.argtypes = [vp, ctypes.POINTER(SceneView)]
    L.frt_shard_slot_count.argtypes = [ctypes.POINTER(RenderParams)]
    L.frt_shard_slot_count.restype = ctypes.c_int64
    L.frt_shard_slots.argtypes = [ctypes.POINTER(RenderParams), vp]
    L.frt_render.argtypes = [vp, ctypes.POINTER(RenderParams), vp, ctypes.POINTER(Stats)]
    L.frt_render_device.argtypes = [vp, ctypes.POINTER(RenderParams), vp, vp, ctypes.POINTER(Stats)]
    L.frt_trace_device.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int, vp, ctypes.POINTER(Stats)]
    L.frt_mlt_chain_state.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, vp, vp]
    L.frt_render_multi.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(RenderParams), vp,
                                   ctypes.POINTER(Stats)]
    L.frt_scene_create.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double, ctypes.POINTER(vp)]
    L.frt_scene_view_get.argtypes = [vp, ctypes.POINTER(SceneView)]
    L.frt_scene_info.argtypes = [vp, ctypes.POINTER(HostSceneInfo)]
    L.frt_scene_destroy.argtypes = [vp]
    L.frt_scene_destroy.restype = None
    dp = ctypes.POINTER(ctypes.c_double)
    L.frt_scene_new.argtypes = [ctypes.POINTER(vp)]
    L.frt_scene_add_obj.argtypes = [vp, ctypes.c_char_p, dp, ctypes.POINTER(Material), ctypes.c_int]
    L.frt_scene_add_sphere.argtypes = [vp, dp, ctypes.c_double, ctypes.POINTER(Material), ctypes.c_int]
    L.frt_scene_set_camera.argtypes = [vp, dp, dp, dp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double]
    L.frt_scene_set_env.argtypes = [vp, dp]
    L.frt_scene_add_image.argtypes = [vp, ctypes.POINTER(Image), ctypes.POINTER(ctypes.c_int)]
    L.frt_scene_finish.argtypes = [vp, ctypes.c_int]
    L.frt_scene_build_bvh_gpu.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_double)]
    L.frt_scene_build_bvh_sah.argtypes = [vp]
    L.frt_scene_build_bvh_gpu_algo.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.frt_write_tessellated_obj.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
    L.frt_write_pfm.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, vp]
    L.frt_film_accumulate.argtypes = [vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int64]
    L.frt_tonemap_u8.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    L.frt_write_image.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int]
    L.frt_selftest_path_host.argtypes = [ctypes.POINTER(SceneView), ctypes.POINTER(RenderParams), vp,
                                         ctypes.c_int, vp, ctypes.POINTER(Stats)]
    L.frt_selftest_mlt_paths_host.argtypes = [ctypes.POINTER(SceneView), ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                                              ctypes.c_int, vp]
    L.frt_set_env_image.argtypes = [vp, ctypes.POINTER(Image)]
    L.frt_scene_set_env_image.argtypes = [vp, ctypes.c_int]
    L.frt_scene_env_image.argtypes = [vp, ctypes.POINTER(Image)]
    L.frt_read_hdr.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), vp]
    L.frt_selftest_path_host_env.argtypes = [ctypes.POINTER(SceneView), ctypes.POINTER(RenderParams), vp,
                                             ctypes.c_int, ctypes.POINTER(Image), vp, ctypes.POINTER(Stats)]
    L.frtx_selftest_tree_refine.argtypes = [ctypes.POINTER(SceneView), ctypes.POINTER(TreeCost), vp, vp, ctypes.c_int32]
    L.frtx_selftest_shadow_tree.argtypes = [ctypes.POINTER(SceneView), ctypes.POINTER(ShadowTreeInfo), vp, vp,
                                            ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32]
    if hasattr(L, "frtx_selftest_exit_tree"):   # (FRT_LIB_PATH may name an earlier revision's build for a timing A/B)
        L.frtx_selftest_exit_tree.argtypes = [ctypes.POINTER(SceneView), ctypes.c_int32, ctypes.POINTER(ExitTreeInfo), vp,
                                              vp, vp, ctypes.c_int32, vp, vp, ctypes.c_int32]
    L.frtx_selftest_trace_host.argtypes = [ctypes.POINTER(SceneView), vp, ctypes.c_int64, vp]
    L.frtx_selftest_chunk_variance.argtypes = [vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp]
    L.frtx_render_pixels.argtypes = [vp, ctypes.POINTER(RenderParams), vp, ctypes.c_int64, vp, vp, ctypes.POINTER(Stats)]
    L.frtx_render_pixels_device.argtypes = [vp, ctypes.POINTER(RenderParams), vp, ctypes.c_int64, vp, vp, vp,
                                            ctypes.POINTER(Stats)]
    if hasattr(L, "frtx_radiance_rays"):   # (FRT_LIB_PATH may name an earlier revision's build for a timing A/B)
        L.frtx_radiance_rays.argtypes = [vp, ctypes.POINTER(RenderParams), vp, ctypes.c_int64, vp, vp, ctypes.POINTER(Stats)]
        L.frtx_radiance_rays_device.argtypes = [vp, ctypes.POINTER(RenderParams), vp, ctypes.c_int64, vp, vp, vp,
                                                ctypes.POINTER(Stats)]
        L.frtx_camera_rays_device.argtypes = [vp, ctypes.POINTER(RenderParams), vp, ctypes.c_int64, vp, vp]
        L.frtx_selftest_radiance_host.argtypes = [ctypes.POINTER(SceneView), ctypes.POINTER(RenderParams), vp, ctypes.c_int64,
                                                  ctypes.POINTER(Image), vp, ctypes.POINTER(Stats)]
        L.frtx_selftest_camera_rays_host.argtypes = [ctypes.POINTER(SceneView), ctypes.POINTER(RenderParams), vp,
                                                     ctypes.c_int64, vp]
    if hasattr(L, "frtx_prt_transfer"):   # (FRT_LIB_PATH may name an earlier revision's build for a timing A/B)
        sv = ctypes.POINTER(SceneView)
        L.frtx_prt_basis.argtypes = [vp, ctypes.c_int64, vp]
        L.frtx_sh_project_image.argtypes = [ctypes.POINTER(Image), vp, vp]
        L.frtx_prt_sample_dirs.argtypes = [ctypes.c_int, ctypes.c_uint32, vp]
        L.frtx_prt_corners.argtypes = [sv, vp, vp]
        L.frtx_prt_transfer.argtypes = [vp, sv, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(Stats)]
        L.frtx_prt_transfer_device.argtypes = [vp, sv, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, vp,
                                               ctypes.POINTER(Stats)]
        L.frtx_prt_rays.argtypes = [vp, vp, vp, vp, ctypes.c_int64, vp, ctypes.POINTER(Stats)]
        L.frtx_prt_rays_device.argtypes = [vp, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.POINTER(Stats)]
        L.frtx_selftest_prt_transfer_host.argtypes = [sv, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp]
        L.frtx_selftest_prt_rays_host.argtypes = [sv, ctypes.POINTER(Image), vp, vp, vp, ctypes.c_int64, vp]
        L.frtx_prt_render.argtypes = [vp, ctypes.POINTER(RenderParams), vp, vp, vp, ctypes.POINTER(Stats)]
        L.frtx_selftest_prt_budget.argtypes = [ctypes.c_int64]
    _lib = L
    return L


def _check(rc, what, ctx=None):
    if rc != 0:
        msg = ""
        if ctx is not None:
            msg = lib().frt_last_error(ctx).decode(errors="replace")
        elif "_rays" in what or "radiance" in what or "prt" in what or "sh_project" in what:   # hooks without a context: frt_last_error(NULL) has their text
            msg = lib().frt_last_error(None).decode(errors="replace")
        raise FrtError(f"{what} failed: {ERRORS.get(rc, rc)} {msg}")


class HostScene:
    """Scene built natively (main.cpp scene constructors + mesh_loader + create_bvh)."""

    def __init__(self, kind, obj_path, aspect):
        self.ptr = ctypes.c_void_p()
        _check(lib().frt_scene_create(kind.encode(), obj_path.encode(), float(aspect), ctypes.byref(self.ptr)),
               f"frt_scene_create({kind})")
        self.info = HostSceneInfo()
        lib().frt_scene_info(self.ptr, ctypes.byref(self.info))
        self.env = None

    def set_env(self, rgb):
        """Constant environment colour of the views this scene hands out
        (material.h:206-232; the reference scenes use black)."""
        self.env = tuple(float(x) for x in rgb)

    def set_env_image(self, index):
        """Image `index` of the scene (spec "images") is its environment map
        (frt_scene_set_env_image); -1 or None = the constant colour again.
        Context.upload() forwards it to the context."""
        _check(lib().frt_scene_set_env_image(self.ptr, -1 if index is None else int(index)), "frt_scene_set_env_image")

    def env_image(self):
        """The scene's environment image as an Image (frt_scene_env_image; its
        data belongs to the scene), or None."""
        img = Image()
        rc = lib().frt_scene_env_image(self.ptr, ctypes.byref(img))
        if rc < 0:
            _check(rc, "frt_scene_env_image")
        return img if rc == 1 else None

    @classmethod
    def from_spec(cls, spec, aspect):
        """Build a scene the way main.cpp's scene functions do (frt_scene_new ...
        frt_scene_finish).  `spec`:
          {"objects": [{"obj": path, "to_world": 16 floats (row-major) | None,
                        "bsdf": material | None, "geo": use_geometry_normals},
                       {"sphere": (x, y, z), "radius": r, "material": material,
                        "where": "world" | "lights" | "both"}, ...],
           "camera": {"lookfrom", "lookat", "vup", "vfov", "aperture", "focus"},
           "world": "bvh" | "list", "env": (r, g, b) | None,
           "images": [{"data": (ny, nx, 3) uint8 sRGB | float32}, ...],
           "env_image": index into "images" (the environment map) | None}
        material: {"type": "lambertian" | "diffuse_light" | "modified_phong" |
                   "metal" | "dielectric" | "rough_conductor", "albedo", "emit",
                   "specular", "exponent", "ior", "alpha", "distribution":
                   "ggx" | "beckmann", "eta", "k", "checker": {"odd", "scale"},
                   "image": index into "images"}.
        oracle.OracleScene.from_spec builds the same scene in the oracle."""
        self = cls.__new__(cls)
        self.ptr = ctypes.c_void_p()
        self.env = None
        L = lib()
        _check(L.frt_scene_new(ctypes.byref(self.ptr)), "frt_scene_new")

        def dptr(x):
            a = np.ascontiguousarray(np.asarray(x, np.float64))
            return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        for img in spec.get("images", ()):   # materials refer to them by index ({"image": i})
            a, fmt = image_array(img)
            desc = Image(a.shape[1], a.shape[0], fmt, 0, a.ctypes.data)
            idx = ctypes.c_int(-1)
            _check(L.frt_scene_add_image(self.ptr, ctypes.byref(desc), ctypes.byref(idx)), "frt_scene_add_image")
        for o in spec["objects"]:
            if "obj" in o:
                tw = dptr(o["to_world"]) if o.get("to_world") is not None else (None, None)
                bs = ctypes.byref(Material.from_spec(o["bsdf"])) if o.get("bsdf") is not None else None
                _check(L.frt_scene_add_obj(self.ptr, o["obj"].encode(), tw[1], bs, int(bool(o.get("geo", False)))),
                       f"frt_scene_add_obj({o['obj']})")
            else:
                c = dptr(o["sphere"])
                _check(L.frt_scene_add_sphere(self.ptr, c[1], float(o["radius"]),
                                              ctypes.byref(Material.from_spec(o["material"])),
                                              SPHERE_WHERE[o.get("where", "world")]), "frt_scene_add_sphere")
        cam = spec["camera"]
        f, a, u = dptr(cam["lookfrom"]), dptr(cam["lookat"]), dptr(cam.get("vup", (0, 1, 0)))
        _check(L.frt_scene_set_camera(self.ptr, f[1], a[1], u[1], float(cam["vfov"]), float(aspect),
                                      float(cam.get("aperture", 0.0)), float(cam.get("focus", 10.0))),
               "frt_scene_set_camera")
        if spec.get("env") is not None:
            e = dptr(spec["env"])
            _check(L.frt_scene_set_env(self.ptr, e[1]), "frt_scene_set_env")
        if spec.get("env_image") is not None:
            _check(L.frt_scene_set_env_image(self.ptr, int(spec["env_image"])), "frt_scene_set_env_image")
        _check(L.frt_scene_finish(self.ptr, {"bvh": 0, "list": 1}[spec.get("world", "bvh")]), "frt_scene_finish")
        self.info = HostSceneInfo()
        L.frt_scene_info(self.ptr, ctypes.byref(self.info))
        return self

    def view(self):
        v = SceneView()
        _check(lib().frt_scene_view_get(self.ptr, ctypes.byref(v)), "frt_scene_view_get")
        if self.env is not None:
            v.env_color[:] = self.env
        return v

    def arrays(self):
        """numpy views of the flattened scene (copies)."""
        v = self.view()

        def arr(ptr, n, dt, w=1):
            if n == 0 or not ptr:
                return np.zeros((0, w) if w > 1 else 0, dt)
            a = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                      shape=(n * w,)).copy()
            return a.reshape(n, w) if w > 1 else a
        return {
            "tri_v": arr(v.tri_v, v.n_tris, np.float64, 9),
            "tri_material": arr(v.tri_material, v.n_tris, np.int32),
            "sphere": arr(v.sphere, v.n_spheres, np.float64, 4),
            "node_box": arr(v.node_box, v.n_nodes, np.float64, 6),
            "node_child": arr(v.node_child, v.n_nodes, np.int32, 2),
            "root": v.root,
            "lights": arr(v.lights, v.n_lights, np.int32),
            "list": arr(v.list, v.n_list, np.int32),
        }

    def build_bvh_sah(self):
        """Replace the world by a binned-SAH tree (frt_scene_build_bvh_sah); returns build ms."""
        _check(lib().frt_scene_build_bvh_sah(self.ptr), "frt_scene_build_bvh_sah")
        lib().frt_scene_info(self.ptr, ctypes.byref(self.info))
        return self.info.build_ms

    def build_bvh_gpu(self, ctx, algo="gsah"):
        """Replace the world by a GPU-built BVH (frt_scene_build_bvh_gpu_algo): "gsah"
        (top-down binned SAH, the default), "ploc" (PLOC clustering) or "lbvh" (Karras
        linear BVH); returns the device time of the build passes in ms."""
        ms = ctypes.c_double()
        a = {"ploc": FRT_GPU_BVH_PLOC, "lbvh": FRT_GPU_BVH_LBVH, "gsah": FRT_GPU_BVH_SAH}[algo]
        _check(lib().frt_scene_build_bvh_gpu_algo(self.ptr, ctx.ptr, a, ctypes.byref(ms)),
               "frt_scene_build_bvh_gpu_algo", ctx.ptr)
        lib().frt_scene_info(self.ptr, ctypes.byref(self.info))
        return ms.value

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                lib().frt_scene_destroy(self.ptr)
            except Exception:
                pass
            self.ptr = None


class Context:
    """One GPU (frt_ctx).  Raises FrtError when no gfx950 device is present."""

    def __init__(self, device=0, precision=None):
        self.ptr = ctypes.c_void_p()
        self.device = int(device)
        _check(lib().frt_create(int(device), ctypes.byref(self.ptr)), f"frt_create(device={device})")
        if precision is not None:
            self.set_precision(precision)

    def set_precision(self, precision):
        """FRT_PRECISION_AUTO / _FP32 / _FP64 (or "auto" / "fp32" / "fp64"); before upload()."""
        if isinstance(precision, str):
            precision = {"auto": FRT_PRECISION_AUTO, "fp32": FRT_PRECISION_FP32, "fp64": FRT_PRECISION_FP64}[precision]
        _check(lib().frt_set_precision(self.ptr, int(precision)), "frt_set_precision", self.ptr)

    def upload(self, scene):
        """frt_upload_scene.  A HostScene with an environment image
        (HostScene.set_env_image / spec "env_image") also sets it on the context; one
        without clears an image that an earlier upload() forwarded.  An image set
        with Context.set_env_image stays until that call changes it."""
        view = scene.view() if isinstance(scene, HostScene) else scene
        _check(lib().frt_upload_scene(self.ptr, ctypes.byref(view)), "frt_upload_scene", self.ptr)
        self._n_tris = int(view.n_tris)   # prt_rays checks the size of its T against it
        img = scene.env_image() if isinstance(scene, HostScene) else None
        if img is not None:
            _check(lib().frt_set_env_image(self.ptr, ctypes.byref(img)), "frt_set_env_image", self.ptr)
            self._env_from_scene = True
        elif isinstance(scene, HostScene) and getattr(self, "_env_from_scene", False):
            _check(lib().frt_set_env_image(self.ptr, None), "frt_set_env_image", self.ptr)
            self._env_from_scene = False

    def set_env_image(self, image):
        """The context's environment map (frt_set_env_image): a (ny, nx, 3)
        uint8 (sRGB) or float32 array, copied to the device and kept across
        upload(); None = the constant env colour of the uploaded scene."""
        self._env_from_scene = False
        if image is None:
            _check(lib().frt_set_env_image(self.ptr, None), "frt_set_env_image", self.ptr)
            return
        a, fmt = image_array({"data": image})
        desc = Image(a.shape[1], a.shape[0], fmt, 0, a.ctypes.data)
        _check(lib().frt_set_env_image(self.ptr, ctypes.byref(desc)), "frt_set_env_image", self.ptr)

    def render(self, params, film=None):
        """Render into a full film (nx*ny*3 float32, y=0 bottom row).  Returns (film, stats)."""
        if film is None:
            film = np.zeros((params.ny, params.nx, 3), np.float32)
        assert film.dtype == np.float32 and film.flags.c_contiguous and film.size == params.nx * params.ny * 3
        st = Stats()
        _check(lib().frt_render(self.ptr, ctypes.byref(params), film.ctypes.data, ctypes.byref(st)),
               "frt_render", self.ptr)
        return film, st

    def denoise(self, film, nx, ny, spp=16, seed=0, tile_size=32, flags=0):
        """FRT_INTEGRATOR_DENOISE: filter the finished colour film (ny, nx, 3) float32 -- finite
        and >= 0 (a path film can hold values a few 1e-6 below 0: np.maximum(film, 0) first), from
        path, accumulated passes or pssmlt -- in place, guided by spp-sample normals, albedo and
        depth renders of the uploaded scene.  Returns (film, stats)."""
        p = RenderParams.make(nx, ny, spp, seed=seed, tile_size=tile_size, flags=flags,
                              integrator=FRT_INTEGRATOR_DENOISE)
        return self.render(p, film=film)

    def render_error(self, params):
        """FRT_INTEGRATOR_ERROR: the variance film V (ny, nx, 3) float32 of the film this context's
        last render produced -- per pixel and channel the batch-means estimate of the variance of
        the mean, from the spread of that render's chunk sums; sqrt(V) is the standard error.
        params: that render's (nx, ny, spp, tile_size and the shard are compared).  Returns (V, stats)."""
        p = RenderParams.from_buffer_copy(params)
        p.integrator = FRT_INTEGRATOR_ERROR
        return self.render(p)

    def render_pixels(self, params, pixels, variance=True):
        """frtx_render_pixels: the pixels of the list (linear indices y * nx + x of the frame of
        `params`; duplicates allowed) through the sparse kernel -- per entry the mean of the
        samples [sample_offset, sample_offset + spp) that render() draws for that pixel, and the
        batch-means V of render_error over chunks of samples_per_item samples (0: spp / 16).
        path and ao.  Leaves the chunk sums of the last render() alone.
        Returns (rgb (n, 3) float32, V (n, 3) float32 or None, stats)."""
        pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
        rgb = np.zeros((len(pixels), 3), np.float32)
        V = np.zeros((len(pixels), 3), np.float32) if variance else None
        st = Stats()
        _check(lib().frtx_render_pixels(self.ptr, ctypes.byref(params), pixels.ctypes.data, len(pixels), rgb.ctypes.data,
                                        V.ctypes.data if variance else None, ctypes.byref(st)),
               "frtx_render_pixels", self.ptr)
        return rgb, V, st

    def radiance_rays(self, params, rays, variance=True):
        """frtx_radiance_rays: the radiance along caller-supplied first rays through this
        library's integrator (path or ao).  rays: (n, 8) float32, frt_trace_device's record --
        origin, t_max of the first segment, direction (any length), and in word 7 the entry's RNG
        stream id as uint32 bits (ray_records() builds them; entries with equal ids share their
        random numbers).  Per entry the mean of Li over samples [sample_offset, sample_offset +
        spp), every sample along the same first ray, and the batch-means V of render_pixels.
        nx, ny and tile_size of `params` are ignored.
        Returns (rgb (n, 3) float32, V (n, 3) float32 or None, stats)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        rgb = np.zeros((len(rays), 3), np.float32)
        V = np.zeros((len(rays), 3), np.float32) if variance else None
        st = Stats()
        _check(lib().frtx_radiance_rays(self.ptr, ctypes.byref(params), rays.ctypes.data, len(rays), rgb.ctypes.data,
                                        V.ctypes.data if variance else None, ctypes.byref(st)),
               "frtx_radiance_rays", self.ptr)
        return rgb, V, st

    def camera_rays(self, params, pixels):
        """frtx_camera_rays_device: the first rays the scene's own camera makes for the listed
        pixels of the nx x ny frame at sample `sample_offset` (fp32; FRT_FLAG_SOBOL selects that
        sampler's film and lens points), as (n, 8) float32 records with the pixel as stream id --
        radiance_rays of them at spp = 1 is render_pixels of the pixels.  The list and the
        records pass through device memory (torch)."""
        import torch
        pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
        dev = torch.device("cuda", self.device)
        px = torch.from_numpy(pixels).to(dev)
        out = torch.zeros((len(pixels), 8), dtype=torch.float32, device=dev)
        _check(lib().frtx_camera_rays_device(self.ptr, ctypes.byref(params), px.data_ptr(), len(pixels), out.data_ptr(), None),
               "frtx_camera_rays_device", self.ptr)
        return out.cpu().numpy()

    def render_camera(self, params, make_rays, passes=1):
        """An image through a camera of the caller's: make_rays(jitter) -> (n, 8) ray records
        (first_raytracer_amd.cameras), jitter a (2,) offset in [0, 1)^2 inside the texel.  Pass k
        of `passes` renders spp samples at sample_offset = k * spp along rays jittered by a pair
        hashed from (seed, k) -- pass 0 of a single pass takes the texel centres -- and the passes
        are combined by film_accumulate's rule.  Returns (rgb (n, 3) float32, stats of the last pass)."""
        acc, st = None, None
        for k in range(int(passes)):
            p = RenderParams.from_buffer_copy(params)
            p.sample_offset = params.sample_offset + k * params.spp
            jitter = None if passes == 1 else np.random.default_rng([int(params.seed), k]).random(2)
            rgb, _, st = self.radiance_rays(p, make_rays(jitter), variance=False)
            acc = rgb if acc is None else film_accumulate(acc, k * params.spp, rgb, params.spp)
        return acc, st

    def prt_transfer(self, scene, dirs, bounces=0, flags=0, budget=None):
        """frtx_prt_transfer: the diffuse transfer vectors of the uploaded scene, T (n_tris, 3, 25, 3)
        float32 -- per triangle corner, SH coefficient and channel --, summed over `bounces`
        interreflections.  scene: the HostScene (or SceneView) that was uploaded; dirs: (n, 3) float32
        unit directions (prt_sample_dirs); flags: FRTX_PRT_UNSHADOWED, FRT_FLAG_BVH2.  budget: bytes
        of chunk sums one batch of corners may take (a test knob; the result does not depend on it).
        Returns (T, stats)."""
        view = _view(scene)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        T = np.zeros((int(view.n_tris), 3, PRT_COEFFS, 3), np.float32)
        st = Stats()
        with _prt_budget(budget):
            _check(lib().frtx_prt_transfer(self.ptr, ctypes.byref(view), dirs.ctypes.data, len(dirs), int(bounces), int(flags),
                                           T.ctypes.data, ctypes.byref(st)), "frtx_prt_transfer", self.ptr)
        return T, st

    def prt_transfer_device(self, scene, dirs, bounces=0, flags=0):
        """frtx_prt_transfer_device: prt_transfer into device memory; returns (T as a torch tensor
        on this context's device, stats)."""
        import torch
        view = _view(scene)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        T = torch.zeros((int(view.n_tris), 3, PRT_COEFFS, 3), dtype=torch.float32, device=torch.device("cuda", self.device))
        st = Stats()
        _check(lib().frtx_prt_transfer_device(self.ptr, ctypes.byref(view), dirs.ctypes.data, len(dirs), int(bounces),
                                              int(flags), T.data_ptr(), None, ctypes.byref(st)),
               "frtx_prt_transfer_device", self.ptr)
        return T, st

    def prt_rays(self, T, li, rays):
        """frtx_prt_rays: PRT shading along rays -- the closest hit of each ((n, 8) float32 records,
        ray_records() / camera_rays() / first_raytracer_amd.cameras), then on a lambertian triangle the
        dot product of li (sh_project_image, (25, 3)) with the transfer T interpolated at the hit, on
        an emitter its emission, on a miss the context's environment.  Returns (rgb (n, 3), stats)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        T = np.ascontiguousarray(T, dtype=np.float32)
        li = np.ascontiguousarray(li, dtype=np.float32).reshape(-1)
        if li.size != 3 * PRT_COEFFS:
            raise ValueError("li: (25, 3) coefficients")
        if hasattr(self, "_n_tris") and T.size != self._n_tris * 9 * PRT_COEFFS:
            raise ValueError("T: (n_tris, 3, 25, 3) of the uploaded scene")
        rgb = np.zeros((len(rays), 3), np.float32)
        st = Stats()
        _check(lib().frtx_prt_rays(self.ptr, T.ctypes.data, li.ctypes.data, rays.ctypes.data, len(rays), rgb.ctypes.data,
                                   ctypes.byref(st)), "frtx_prt_rays", self.ptr)
        return rgb, st

    def render_prt(self, params, T, li, make_rays=None):
        """A PRT image: per sample s of params.spp the camera's first rays (camera_rays at sample
        sample_offset + s: the film and lens points a path render takes) shaded by prt_rays, the
        samples averaged by film_accumulate's rule.  make_rays(jitter) -> (n, 8) records, a camera of
        first_raytracer_amd.cameras, replaces the scene's camera (jitter hashed from (seed, s), the
        texel centres for a single sample).  Returns (film (ny, nx, 3) float32, y = 0 the bottom row
        -- with make_rays (n, 3) in the camera's order --, stats of the last sample)."""
        T = np.ascontiguousarray(T, dtype=np.float32)
        li = np.ascontiguousarray(li, dtype=np.float32).reshape(-1)
        if li.size != 3 * PRT_COEFFS or (hasattr(self, "_n_tris") and T.size != self._n_tris * 9 * PRT_COEFFS):
            raise ValueError("T: (n_tris, 3, 25, 3) of the uploaded scene, li: (25, 3)")
        st = Stats()
        if make_rays is None:   # frtx_prt_render: the same composition inside the library
            film = np.zeros((params.ny, params.nx, 3), np.float32)
            _check(lib().frtx_prt_render(self.ptr, ctypes.byref(params), T.ctypes.data, li.ctypes.data, film.ctypes.data,
                                         ctypes.byref(st)), "frtx_prt_render", self.ptr)
            return film, st
        acc = None
        for s in range(int(params.spp)):
            rays = make_rays(None if params.spp == 1 else np.random.default_rng([int(params.seed), s]).random(2))
            rgb, st = self.prt_rays(T, li, rays)
            acc = rgb if acc is None else film_accumulate(acc, s, rgb, 1)
        return acc, st

    def render_until(self, params, target, max_spp, first_spp=None, adaptive=False, switch=None):
        """Progressive render of `params` (path or ao; spp and sample_offset are the driver's) that
        stops at a requested error instead of a guessed sample count.  The frame figure is
        e = sqrt(mean V) / mean film (frame_error): the predicted RMSE of the film over its mean.
        Pass 0 renders first_spp samples (a power of two >= 2; None: 16, or ADAPTIVE_FIRST_SPP for
        an adaptive run), each later pass as many as there are so far; the film is accumulated with film_accumulate and V combined with
        combine_variance (the passes are independent).  The loop ends when e <= target (converged)
        or when the next pass would exceed max_spp.  With FRT_FLAG_SOBOL the samples of a pixel
        are one net and V says nothing about its error: four replicates (seeds seed .. seed + 3)
        are each extended by the same passes, the film is their mean and V the sample variance
        of the four replicate means / 4 (replicate_variance); spp_used counts all four.
        Returns (film, V, spp_used, e, converged).
        adaptive=True: the later passes sample only the pixels whose own error is above the
        target (render_until's rule; render_pixels when their share is below `switch`);
        returns (film, V, counts, e, converged) with counts the (ny, nx) int32 samples per pixel."""
        if adaptive:
            film, V, counts, e, ok, _ = render_until(lambda p: self.render(p), lambda p: self.render_error(p)[0],
                                                     params, target, max_spp, first_spp, adaptive=True,
                                                     render_pixels=lambda p, px: self.render_pixels(p, px), switch=switch)
            return film, V, counts, e, ok
        film, V, spp, e, ok, _ = render_until(lambda p: self.render(p), lambda p: self.render_error(p)[0],
                                              params, target, max_spp, first_spp)
        return film, V, spp, e, ok

    def render_device(self, params, dev_ptr, stream_ptr=None):
        """Render this shard's slots into device memory at dev_ptr (slot_count*3 floats)."""
        st = Stats()
        _check(lib().frt_render_device(self.ptr, ctypes.byref(params), ctypes.c_void_p(dev_ptr),
                                       ctypes.c_void_p(stream_ptr) if stream_ptr else None, ctypes.byref(st)),
               "frt_render_device", self.ptr)
        return st

    def mlt_chain_state(self, first, n):
        """Local chains [first, first + n) of the last PSS-MLT render: (final
        states n x 92 float32, fingerprints n x 2 uint32 = accepted proposals,
        sum of the accepted steps' 1-based indices mod 2^32)."""
        u = np.zeros((max(n, 1), 92), np.float32)
        fp = np.zeros((max(n, 1), 2), np.uint32)
        _check(lib().frt_mlt_chain_state(self.ptr, int(first), int(n), u.ctypes.data, fp.ctypes.data),
               "frt_mlt_chain_state", self.ptr)
        return u[:n], fp[:n]

    def trace_device(self, rays_ptr, n, hits_ptr, flags=0, stream_ptr=None):
        """Batched Scene::world->hit on device buffers: rays n x 8 floats (origin, t_max,
        direction, flags bit 0 = any hit), hits n x 4 (t, u, v, prim bits).  Returns stats."""
        st = Stats()
        _check(lib().frt_trace_device(self.ptr, ctypes.c_void_p(rays_ptr), int(n), ctypes.c_void_p(hits_ptr), int(flags),
                                      ctypes.c_void_p(stream_ptr) if stream_ptr else None, ctypes.byref(st)),
               "frt_trace_device", self.ptr)
        return st

    def close(self):
        if getattr(self, "ptr", None):
            lib().frt_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_multi(contexts, params, film=None):
    """One process, several GPUs (frt_render_multi): contexts[i] renders shard
    (i, n) of the whole-frame `params` on its own host thread.  Returns (film, stats)."""
    if film is None:
        film = np.zeros((params.ny, params.nx, 3), np.float32)
    assert film.dtype == np.float32 and film.flags.c_contiguous and film.size == params.nx * params.ny * 3
    arr = (ctypes.c_void_p * len(contexts))(*[c.ptr for c in contexts])
    st = Stats()
    _check(lib().frt_render_multi(arr, len(contexts), ctypes.byref(params), film.ctypes.data, ctypes.byref(st)),
           "frt_render_multi", contexts[0].ptr)
    return film, st


def frame_error(film, V):
    """The frame figure of render_until: e = sqrt(mean V) / mean film, both means over all
    3 nx ny values, in float64.  (frt::frame_error adds the same values one after the other:
    the two agree to rounding, not bit for bit; the films of the two drivers do.)"""
    f = np.asarray(film, np.float64)
    v = np.asarray(V, np.float64)
    return float(np.sqrt(v.sum() / v.size) / (f.sum() / f.size))


def combine_variance(a, Va, b, Vb):
    """Variance film of the mean of a + b samples from the variance films of the means of the
    first a and the other b (independent passes): (a^2 Va + b^2 Vb) / (a + b)^2, in float64,
    stored as float32."""
    a, b = float(a), float(b)
    va, vb = np.asarray(Va, np.float64), np.asarray(Vb, np.float64)
    return (((a * a) * va + (b * b) * vb) / ((a + b) * (a + b))).astype(np.float32)


def replicate_variance(films):
    """(mean film float32, V float32) of four replicate films: V = the sample variance of the
    four replicate means / 4, in float64 (np.var(films, axis=0, ddof=1) / 4); the mean film
    through film_accumulate, one replicate at a time."""
    assert len(films) == 4
    r = [np.asarray(f, np.float64) for f in films]
    m = (((r[0] + r[1]) + r[2]) + r[3]) * 0.25
    v = ((((r[0] - m) ** 2 + (r[1] - m) ** 2) + (r[2] - m) ** 2) + (r[3] - m) ** 2) / 12.0
    mean = np.array(films[0], np.float32, copy=True)
    for k in range(1, 4):
        mean = film_accumulate(mean, k, films[k], 1)
    return mean, v.astype(np.float32)


# The active share of the frame below which an adaptive pass goes through render_pixels: the
# full render's time over the sparse kernel's for the same pixels and samples, rounded down to
# one decimal (1080p, 64 spp, one MI355X: profiles/adaptive/switch.json).
ADAPTIVE_SWITCH = 0.5
# The first pass of an adaptive run when the caller names none: the smallest power of two at which
# the run's sum of mean V stays inside the calibration window of the sum of the actual squared
# error (tools/adaptive_calibration.py, profiles/adaptive/calibration.json)
ADAPTIVE_FIRST_SPP = 128


def frame_mean(film):
    """Mean of all 3 nx ny film values, added one after the other in float64 (np.cumsum adds in
    order): the sum frt::render_until's adaptive rule forms, bit for bit."""
    f = np.asarray(film, np.float64).reshape(-1)
    return float(np.cumsum(f)[-1] / f.size)


def render_until(render, render_error, params, target, max_spp, first_spp=None, adaptive=False, render_pixels=None,
                 switch=None):
    """The loop of Context.render_until over callables: render(params) -> (film, stats) and
    render_error(params) -> V of the render just done.  Returns (film, V, spp_used, e,
    converged, passes) with passes = [(spp_used, e, kernel ms of the pass)].
    A pass whose render cut the samples into one chunk (stats.work_items equals the slot
    count; the granule depends on the device, so it is seen only after the render) has no
    spread to estimate from: it is rendered again with samples_per_item = half the pass --
    that pass is paid twice -- and every later pass asks for half-pass granules up front.

    adaptive=True (render_pixels(params, pixels) -> (rgb, V, stats) of the listed pixels): after
    every pass tau = target x the film's mean (frame_mean), and a pixel is active while the mean
    of its three V exceeds tau^2, i.e. sqrt(mean_c V) > tau.  Pass 0 is the full render of
    first_spp samples; a later pass gives every active pixel as many samples as it has (n for
    the most-sampled one), from the first sample index not yet handed out -- so sample_offset =
    spp = n while the active pixels share one count -- through render_pixels when the active
    share of the frame is below `switch` (default ADAPTIVE_SWITCH), else through the full render
    of n samples, after which every pixel holds the new samples.  Per pixel the film merges as film_accumulate and V as
    combine_variance, with that pixel's own count.  The loop ends when no pixel is active --
    then mean V <= tau^2 and e <= target -- or when the next pass would take an active pixel
    past max_spp (2 n > max_spp).  A pixel that stops on its own V is biased: pixels whose first
    samples happen to agree stop early with a V that is too small, so the run's e is optimistic
    unless first_spp is large (DESIGN.md 5d has the measured size; hence ADAPTIVE_FIRST_SPP).  FRT_FLAG_SOBOL is
    refused: V is an upper estimate there and the replicates give no per-pixel figure.
    Returns (film, V, counts, e, converged, passes): counts the (ny, nx) int32 samples per
    pixel, passes = [(samples over the frame so far, e, kernel ms, pixels the pass sampled,
    whether it went through render_pixels)]."""
    if first_spp is None:        # 16; an adaptive run: ADAPTIVE_FIRST_SPP
        first_spp = ADAPTIVE_FIRST_SPP if adaptive else 16
    first_spp, max_spp = int(first_spp), int(max_spp)
    if first_spp < 2 or first_spp & (first_spp - 1):
        raise FrtError("render_until: first_spp must be a power of two >= 2")
    if params.integrator not in (FRT_INTEGRATOR_PATH, FRT_INTEGRATOR_AO):
        raise FrtError("render_until: path and ao renders only (pssmlt has no error estimate, denoise is a filter)")
    if not target > 0:
        raise FrtError("render_until: target must be > 0")
    sobol = bool(params.flags & FRT_FLAG_SOBOL) and params.integrator == FRT_INTEGRATOR_PATH
    reps = 4 if sobol else 1
    if max_spp < reps * first_spp:
        raise FrtError("render_until: max_spp is below the first pass")
    slots = lib().frt_shard_slot_count(ctypes.byref(params))
    if slots < 0:
        raise FrtError("bad render params")
    if adaptive:
        if sobol:
            raise FrtError("render_until: adaptive with FRT_FLAG_SOBOL is refused -- V is an upper estimate under "
                           "Sobol' points and the replicates give no per-pixel error; render without the flag")
        if render_pixels is None:
            raise FrtError("render_until: adaptive needs a render_pixels callable")
        return _render_until_adaptive(render, render_error, render_pixels, params, float(target), max_spp, first_spp,
                                      slots, ADAPTIVE_SWITCH if switch is None else float(switch))
    films, V, total, passes = [None] * reps, None, 0, []
    halve = False
    while True:
        n = first_spp if total == 0 else total
        ms = 0.0
        for k in range(reps):
            p = RenderParams.from_buffer_copy(params)
            p.spp, p.sample_offset, p.seed = n, total, (params.seed + k) & 0xffffffff
            if halve:
                p.samples_per_item = n // 2
            film, st = render(p)
            if not sobol and st.work_items == slots:        # one chunk a pixel
                halve = True
                p.samples_per_item = n // 2
                film, st = render(p)
            ms += st.kernel_ms
            if not sobol:
                Vp = render_error(p)
                V = Vp if total == 0 else combine_variance(total, V, n, Vp)
            films[k] = film if total == 0 else film_accumulate(films[k], total, film, n)
        total += n
        if sobol:
            film, V = replicate_variance(films)
        else:
            film = films[0]
        e = frame_error(film, V)
        passes.append((reps * total, e, ms))
        if e <= target:
            return film, V, reps * total, e, True, passes
        if reps * 2 * total > max_spp:
            return film, V, reps * total, e, False, passes


def _render_until_adaptive(render, render_error, render_pixels, params, target, max_spp, first_spp, slots, switch):
    nx, ny = params.nx, params.ny
    npx = nx * ny
    halve = False

    def full_pass(n, offset):
        nonlocal halve
        p = RenderParams.from_buffer_copy(params)
        p.spp, p.sample_offset = n, offset
        if halve:
            p.samples_per_item = n // 2
        film, st = render(p)
        if st.work_items == slots:        # one chunk a pixel
            halve = True
            p.samples_per_item = n // 2
            film, st = render(p)
        return film, np.asarray(render_error(p), np.float32), st.kernel_ms

    def merge(film_px, V_px, cnt_px, rgb, Vp, n):
        # (k, 3) values of k pixels: one film_accumulate / combine_variance per distinct count
        for c in np.unique(cnt_px):
            g = cnt_px == c
            film_px[g] = film_accumulate(film_px[g], int(c), rgb[g], n)
            V_px[g] = combine_variance(int(c), V_px[g], n, Vp[g])

    film, V, ms = full_pass(first_spp, 0)
    film = np.array(film, np.float32).reshape(npx, 3)
    V = np.array(V, np.float32).reshape(npx, 3)
    counts = np.full(npx, first_spp, np.int64)
    offset = first_spp                    # samples [0, offset) of a pixel's stream are handed out
    passes, sampled, sparse = [], npx, False
    while True:
        tau = target * frame_mean(film)
        v64 = V.astype(np.float64)
        active = np.flatnonzero(((v64[:, 0] + v64[:, 1]) + v64[:, 2]) / 3.0 > tau * tau)
        e = frame_error(film, V)
        passes.append((int(counts.sum()), e, ms, sampled, sparse))
        done = len(active) == 0
        n = 0 if done else int(counts[active].max())      # the pass to come doubles the active pixels
        if done or 2 * n > max_spp:
            return (film.reshape(ny, nx, 3), V.reshape(ny, nx, 3), counts.astype(np.int32).reshape(ny, nx), e, done,
                    passes)
        sparse = len(active) < switch * npx
        if sparse:
            # one call per count among the active pixels, each doubling its group: after sparse
            # passes alone that is one call with sample_offset = spp = n; a pixel that stopped
            # and is active again (tau moves with the film's mean) doubles its smaller count
            ms, before = 0.0, counts[active]
            for c in np.unique(before):
                idx = active[before == c]
                p = RenderParams.from_buffer_copy(params)
                p.spp, p.sample_offset, p.samples_per_item = int(c), offset, 0
                rgb, Vp, st = render_pixels(p, idx.astype(np.int32))
                ms += st.kernel_ms
                film[idx] = film_accumulate(film[idx], int(c), np.asarray(rgb, np.float32), int(c))
                V[idx] = combine_variance(int(c), V[idx], int(c), np.asarray(Vp, np.float32))
                counts[idx] += c
            sampled = len(active)
        else:
            rgb, Vp, ms = full_pass(n, offset)
            merge(film, V, counts, np.asarray(rgb, np.float32).reshape(npx, 3), Vp.reshape(npx, 3), n)
            counts += n
            sampled = npx
        offset += n


def selftest_chunk_variance(partial, spp, spi):
    """FRT_INTEGRATOR_ERROR's arithmetic on the host (frtx_selftest_chunk_variance): partial
    (n_chunks, n_slots, 3) float32 chunk sums, chunks of spi samples, the last what is left of
    spp -> V (n_slots, 3) float32."""
    partial = np.ascontiguousarray(partial, dtype=np.float32)
    k, n, three = partial.shape
    assert three == 3
    out = np.zeros((n, 3), np.float32)
    _check(lib().frtx_selftest_chunk_variance(partial.ctypes.data, k, n, int(spp), int(spi), out.ctypes.data),
           "frtx_selftest_chunk_variance")
    return out


def shard_slots(params):
    """Linear film index (y*nx+x) held by each output slot of a shard (-1 = padding)."""
    n = lib().frt_shard_slot_count(ctypes.byref(params))
    if n < 0:
        raise FrtError("bad render params")
    out = np.zeros(n, np.int32)
    _check(lib().frt_shard_slots(ctypes.byref(params), out.ctypes.data), "frt_shard_slots")
    return out


def selftest_path_host(scene, params, pixels, env_image=None):
    """Self-test hook: the megakernel's per-lane path code run on the host
    (CPU unit tests of the device logic; never a render path).  env_image: a
    (ny, nx, 3) uint8 / float32 environment map, read as a render reads it."""
    pixels = np.ascontiguousarray(pixels, dtype=np.int32)
    out = np.zeros((len(pixels), 3), np.float32)
    st = Stats()
    view = scene.view()
    if env_image is None:
        _check(lib().frt_selftest_path_host(ctypes.byref(view), ctypes.byref(params), pixels.ctypes.data, len(pixels),
                                            out.ctypes.data, ctypes.byref(st)), "frt_selftest_path_host")
        return out, st
    a, fmt = image_array({"data": env_image})
    desc = Image(a.shape[1], a.shape[0], fmt, 0, a.ctypes.data)
    _check(lib().frt_selftest_path_host_env(ctypes.byref(view), ctypes.byref(params), pixels.ctypes.data, len(pixels),
                                            ctypes.byref(desc), out.ctypes.data, ctypes.byref(st)),
           "frt_selftest_path_host_env")
    return out, st


def ray_records(origins, directions, t_max=None, streams=None):
    """(n, 8) float32 ray records for Context.radiance_rays / trace_device: origins and
    directions (n, 3) (either may be one row for all), t_max (scalar or (n,); None: FLT_MAX, the
    camera rays' own), streams (n,) uint32 RNG stream ids (None: arange(n))."""
    o, d = np.broadcast_arrays(np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(directions, np.float32).reshape(-1, 3))
    rec = np.zeros((len(d), 8), np.float32)
    rec[:, 0:3] = o
    rec[:, 3] = np.finfo(np.float32).max if t_max is None else t_max
    rec[:, 4:7] = d
    ids = np.arange(len(d), dtype=np.uint32) if streams is None else np.asarray(streams, np.uint32).reshape(-1)
    rec.view(np.uint32)[:, 7] = ids
    return rec


def selftest_radiance_host(scene, params, rays, env_image=None):
    """Context.radiance_rays through the same per-lane code on the host (frtx_selftest_radiance_host):
    the refusals of the entry point, then ray_begin and the host replay's loop.  Returns (rgb, stats)."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    out = np.zeros((len(rays), 3), np.float32)
    st = Stats()
    view = scene.view()
    desc = None
    if env_image is not None:
        a, fmt = image_array({"data": env_image})
        desc = ctypes.byref(Image(a.shape[1], a.shape[0], fmt, 0, a.ctypes.data))
    _check(lib().frtx_selftest_radiance_host(ctypes.byref(view), ctypes.byref(params), rays.ctypes.data, len(rays), desc,
                                             out.ctypes.data, ctypes.byref(st)), "frtx_selftest_radiance_host")
    return out, st


def _view(scene):
    """The SceneView of a HostScene, or the view itself."""
    return scene.view() if hasattr(scene, "view") else scene


class _prt_budget:
    """The batch budget of prt_transfer and its replay in bytes (frtx_selftest_prt_budget) for the calls inside."""

    def __init__(self, budget):
        self.budget = budget

    def __enter__(self):
        if self.budget is not None:
            _check(lib().frtx_selftest_prt_budget(int(self.budget)), "frtx_selftest_prt_budget")

    def __exit__(self, *exc):
        if self.budget is not None:
            lib().frtx_selftest_prt_budget(0)


def prt_basis(dirs):
    """frtx_prt_basis: Y (n, 25) float32 of unit directions (n, 3) -- the real SH basis in the
    environment image's convention, fp64 rounded once: the table prt_transfer reads."""
    dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    Y = np.zeros((len(dirs), PRT_COEFFS), np.float32)
    _check(lib().frtx_prt_basis(dirs.ctypes.data, len(dirs), Y.ctypes.data), "frtx_prt_basis")
    return Y


def sh_project_image(image=None, env_color=None):
    """frtx_sh_project_image: li (25, 3) float64 of an environment image ((ny, nx, 3) uint8 sRGB or
    float32) or, without one, of the constant colour."""
    li = np.zeros((PRT_COEFFS, 3), np.float64)
    if image is None:
        e = np.ascontiguousarray(env_color, dtype=np.float64).reshape(3)
        _check(lib().frtx_sh_project_image(None, e.ctypes.data, li.ctypes.data), "frtx_sh_project_image")
        return li
    a, fmt = image_array({"data": image})
    desc = Image(a.shape[1], a.shape[0], fmt, 0, a.ctypes.data)
    _check(lib().frtx_sh_project_image(ctypes.byref(desc), None, li.ctypes.data), "frtx_sh_project_image")
    return li


def prt_sample_dirs(sqrt_n, seed=0):
    """frtx_prt_sample_dirs: (sqrt_n^2, 3) float32 unit directions, one per jittered stratum,
    uniform on the sphere."""
    dirs = np.zeros((int(sqrt_n) ** 2 if sqrt_n >= 1 else 1, 3), np.float32)
    _check(lib().frtx_prt_sample_dirs(int(sqrt_n), int(seed), dirs.ctypes.data), "frtx_prt_sample_dirs")
    return dirs


def prt_corners(scene):
    """frtx_prt_corners: (origin (n_tris, 3, 3), normal (n_tris, 3, 3), albedo (n_tris, 3, 3)) float32,
    the corner records prt_transfer traces from."""
    view = _view(scene)
    on = np.zeros((int(view.n_tris), 3, 8), np.float32)
    rho = np.zeros((int(view.n_tris), 3, 3), np.float32)
    _check(lib().frtx_prt_corners(ctypes.byref(view), on.ctypes.data, rho.ctypes.data), "frtx_prt_corners")
    return on[..., 0:3].copy(), on[..., 4:7].copy(), rho


def selftest_prt_transfer_host(scene, dirs, bounces=0, flags=0, budget=None):
    """Context.prt_transfer through the same code on the host (frtx_selftest_prt_transfer_host):
    T (n_tris, 3, 25, 3) float32.  T is created filled with NaN: a refused call writes nothing."""
    view = _view(scene)
    dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    T = np.full((int(view.n_tris), 3, PRT_COEFFS, 3), np.nan, np.float32)
    with _prt_budget(budget):
        _check(lib().frtx_selftest_prt_transfer_host(ctypes.byref(view), dirs.ctypes.data, len(dirs), int(bounces), int(flags),
                                                     T.ctypes.data), "frtx_selftest_prt_transfer_host")
    return T


def selftest_prt_rays_host(scene, T, li, rays, env_image=None):
    """Context.prt_rays through the same code on the host (frtx_selftest_prt_rays_host): rgb (n, 3)."""
    view = _view(scene)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    T = np.ascontiguousarray(T, dtype=np.float32)
    li = np.ascontiguousarray(li, dtype=np.float32).reshape(-1)
    if li.size != 3 * PRT_COEFFS or T.size != int(view.n_tris) * 9 * PRT_COEFFS:
        raise ValueError("T: (n_tris, 3, 25, 3) of the scene, li: (25, 3)")
    rgb = np.zeros((len(rays), 3), np.float32)
    desc = None
    if env_image is not None:
        a, fmt = image_array({"data": env_image})
        desc = ctypes.byref(Image(a.shape[1], a.shape[0], fmt, 0, a.ctypes.data))
    _check(lib().frtx_selftest_prt_rays_host(ctypes.byref(view), desc, T.ctypes.data, li.ctypes.data, rays.ctypes.data,
                                             len(rays), rgb.ctypes.data), "frtx_selftest_prt_rays_host")
    return rgb


def selftest_camera_rays_host(scene, params, pixels):
    """Context.camera_rays on the host (frtx_selftest_camera_rays_host): (n, 8) float32 records."""
    pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
    out = np.zeros((len(pixels), 8), np.float32)
    view = scene.view()
    _check(lib().frtx_selftest_camera_rays_host(ctypes.byref(view), ctypes.byref(params), pixels.ctypes.data, len(pixels),
                                                out.ctypes.data), "frtx_selftest_camera_rays_host")
    return out


def selftest_tree_refine(scene):
    """Counting hook of the tree refinement pass (FRT_TREE_REFINE): the scene
    flattened without and with the pass.  Returns ((cost_off, nodes_off),
    (cost_on, nodes_on)): the TreeCost fields as a dict and the flattened node
    records as an (n_nodes, 16) float32 array (child refs: columns 12, 13 viewed
    as int32)."""
    view = scene.view()
    cap = max(1, view.n_tris + view.n_spheres)
    nodes = [np.zeros((cap, 16), np.float32) for _ in range(2)]
    out = (TreeCost * 2)()
    _check(lib().frtx_selftest_tree_refine(ctypes.byref(view), out, nodes[0].ctypes.data, nodes[1].ctypes.data, cap),
           "frtx_selftest_tree_refine")
    return tuple((out[k].as_dict(), nodes[k][:out[k].n_nodes].copy()) for k in range(2))


def selftest_shadow_tree(scene, segments=0, seed=1):
    """The counting hook of the shadow-tree pass: (info dict, dropped, nodes) -- the
    frt_shadow_tree_info fields, one byte per scene-view triangle (1 = no area-light shadow
    segment can hit it) and the flattened node records, the shadow tree's own behind the main
    tree's nodes_main."""
    view = scene.view()
    cap = max(2 * int(view.n_nodes), 1) + 4
    nodes = np.zeros((cap, 16), np.float32)
    dropped = np.zeros(max(int(view.n_tris), 1), np.uint8)
    out = ShadowTreeInfo()
    _check(lib().frtx_selftest_shadow_tree(ctypes.byref(view), ctypes.byref(out), dropped.ctypes.data, nodes.ctypes.data,
                                           cap, int(segments), int(seed)), "frtx_selftest_shadow_tree")
    return out.as_dict(), dropped[:int(view.n_tris)].copy(), nodes[:out.n_nodes].copy()


EXIT_WHY = ("ran", "off", "material", "not_resident", "too_large", "nothing", "budget")


def selftest_exit_tree(scene, mode=1):
    """The counting hook of the exit-tree pass: (info dict, roots, taken, nodes_off, nodes_on) -- the
    frt_exit_tree_info fields (`why_name`, and `view_of`: device triangle -> scene-view triangle, added),
    per scene-view triangle the node its extension rays start at (0 = the main root), one row (sub, root, members, dropped, added, shared) per drop set
    taken, and the flattened node records without the pass and with it (mode: -1 as FRT_EXIT_TREE
    says, 0 off, 1 on)."""
    view = scene.view()
    cap = max(4 * int(view.n_nodes), 1) + 16
    nodes = np.zeros((2, cap, 16), np.float32)
    roots = np.zeros(max(int(view.n_tris), 1), np.int32)
    taken = np.zeros((64, 6), np.int32)
    view_of = np.zeros(max(int(view.n_tris), 1), np.int32)
    out = ExitTreeInfo()
    _check(lib().frtx_selftest_exit_tree(ctypes.byref(view), int(mode), ctypes.byref(out), roots.ctypes.data,
                                         view_of.ctypes.data, taken.ctypes.data, len(taken), nodes[0].ctypes.data, nodes[1].ctypes.data, cap),
           "frtx_selftest_exit_tree")
    info = out.as_dict()
    info["why_name"] = EXIT_WHY[out.why]
    info["view_of"] = view_of[:int(view.n_tris)].copy()
    return (info, roots[:int(view.n_tris)].copy(), taken[:min(out.taken, len(taken))].copy(),
            nodes[0, :out.nodes_off].copy(), nodes[1, :out.n_nodes].copy())


def selftest_trace_host(scene, rays):
    """Context.trace_device's queries through the same code on the host: rays
    (n, 8) float32 as for frt_trace_device -> hits (n, 4) float32."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    hits = np.zeros((len(rays), 4), np.float32)
    view = scene.view()
    _check(lib().frtx_selftest_trace_host(ctypes.byref(view), rays.ctypes.data, len(rays), hits.ctypes.data),
           "frtx_selftest_trace_host")
    return hits


_handles = None


def kernel_handles():
    """{symbol value: name} of the library's kernel handles, from its symbol table (`nm`): a
    kernel's host-side handle carries the kernel's mangled name, beside its launch stub
    `__device_stub__<name>`."""
    global _handles
    if _handles is None:
        import re
        import subprocess
        out = subprocess.run(["nm", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
        syms = [l.split() for l in out.splitlines()]
        stub = re.compile(r"(\d+)__device_stub__")
        kernels = {stub.sub(lambda m: str(int(m.group(1)) - 15), f[2]) for f in syms if len(f) == 3 and stub.search(f[2])}
        _handles = {int(f[0], 16): f[2] for f in syms if len(f) == 3 and f[2] in kernels}
    return _handles


def selftest_plan(**query):
    """The launch plan of a call without a device (frtx_selftest_plan): query = PlanQuery
    fields.  Returns the PlanAnswer fields as a dict, the kernels by name (None: no kernel, or a
    handle the symbol table does not name)."""
    f = lib().frtx_selftest_plan
    f.argtypes = [ctypes.POINTER(PlanQuery), ctypes.POINTER(PlanAnswer)]
    a = PlanAnswer()
    _check(f(ctypes.byref(PlanQuery(**query)), ctypes.byref(a)), "frtx_selftest_plan")
    d = {n: getattr(a, n) for n, _ in a._fields_}
    for k in ("kernel", "kernel_boot"):
        d[k] = kernel_handles().get(d[k]) if d[k] else None
    return d


def selftest_mlt_paths_host(scene, nx, ny, seed, n):
    """Self-test hook: n PSS-MLT bootstrap eye paths through the device code on the host."""
    out = np.zeros((n, 6), np.float32)
    view = scene.view()
    _check(lib().frt_selftest_mlt_paths_host(ctypes.byref(view), nx, ny, seed, n, out.ctypes.data),
           "frt_selftest_mlt_paths_host")
    return out


def read_hdr(path):
    """Radiance RGBE (.hdr) file -> (ny, nx, 3) float32, rows top to bottom
    (frt_read_hdr: what the reference's image(file, STBI_HDR) holds)."""
    nx, ny = ctypes.c_int32(0), ctypes.c_int32(0)
    _check(lib().frt_read_hdr(os.fsencode(path), ctypes.byref(nx), ctypes.byref(ny), None), f"frt_read_hdr({path})")
    out = np.zeros((ny.value, nx.value, 3), np.float32)
    _check(lib().frt_read_hdr(os.fsencode(path), ctypes.byref(nx), ctypes.byref(ny), out.ctypes.data),
           f"frt_read_hdr({path})")
    return out


def write_pfm(path, film):
    film = np.ascontiguousarray(film, dtype=np.float32)
    ny, nx = film.shape[0], film.shape[1]
    _check(lib().frt_write_pfm(path.encode(), nx, ny, film.ctypes.data), "frt_write_pfm")


def film_accumulate(acc, acc_spp, film, spp):
    """Progressive accumulation (frt_film_accumulate): acc <- mean over acc_spp + spp samples."""
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    film = np.ascontiguousarray(film, dtype=np.float32)
    _check(lib().frt_film_accumulate(acc.ctypes.data, int(acc_spp), film.ctypes.data, int(spp), film.size),
           "frt_film_accumulate")
    return acc


def tonemap_u8(film):
    """viewer::add_sample's display mapping (viewer.cpp:115-117) of a (ny, nx, 3) mean film."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    ny, nx = film.shape[0], film.shape[1]
    out = np.zeros((ny, nx, 3), np.uint8)
    _check(lib().frt_tonemap_u8(film.ctypes.data, nx, ny, out.ctypes.data), "frt_tonemap_u8")
    return out


IMAGE_FORMATS = {"png": 0, "bmp": 1, "jpg": 2}


def write_image(path, rgb_u8, fmt="png"):
    """image::save_image (image.cpp:24-58) of a (ny, nx, 3) u8 image, y = 0 bottom."""
    rgb_u8 = np.ascontiguousarray(rgb_u8, dtype=np.uint8)
    ny, nx = rgb_u8.shape[0], rgb_u8.shape[1]
    _check(lib().frt_write_image(path.encode(), nx, ny, rgb_u8.ctypes.data, IMAGE_FORMATS[fmt]), "frt_write_image")


def work_granule(integrator, spp, n_slots, lanes, spi_req=0):
    """The render's work granule rule (frt_render.hip work_granule; an internal
    symbol of libfrt.so, for host tests): (samples per item, chunks)."""
    L = lib()
    f = L.frt_internal_work_granule
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    spi, k = ctypes.c_int(0), ctypes.c_int(0)
    _check(f(integrator, spp, n_slots, lanes, spi_req, ctypes.byref(spi), ctypes.byref(k)), "work_granule")
    return spi.value, k.value


def write_tessellated_obj(src_obj, k, dst_obj):
    _check(lib().frt_write_tessellated_obj(src_obj.encode(), int(k), dst_obj.encode()), "frt_write_tessellated_obj")
