// frt_kernels.hpp -- the device side shared by the library's kernel units: the
// LDS budgets, the work descriptors, the scene copy into LDS and the
// persistent kernels (path / AO / normals megakernel, ray queries, PSS-MLT
// bootstrap and chains).  Templates only: a unit emits the kernels it
// instantiates (frt_plans.hpp) and nothing else.  The unnamed namespace is
// part of the kernels' symbol names.
//
// One lane owns one path.  Each loop iteration every active lane traces ONE
// ray (camera/extension = closest hit, or shadow = any hit) through the BVH
// with a per-lane LDS stack, then shades.  Lanes whose sample finished start
// the next sample of their work item; lanes whose item finished fetch a new
// one with one wave-aggregated atomic (__ballot + mbcnt compaction).  Work
// items are (tile, sample chunk, 64-pixel block) so a refill hands adjacent
// pixels to the lanes of a wave.  Results are written per (chunk, slot) and
// reduced in a fixed order: the image is deterministic and independent of
// scheduling and of the number of GPUs.
//
// Reference (first_ray/): path::Li path.cpp:4-116, path::Render path.cpp:118-148,
// parallel_bvh_node::hit parallel_bvh.h:39-64, hitable_list::hit
// hitable_list.cpp:4-21, camera::get_ray camera.h:30-35, viewer::add_sample
// viewer.cpp:109-132.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "frt.h"
#include "frt_device.hpp"
#include "frt_path.hpp"
#include "frt_mlt.hpp"

using namespace frt;

namespace {

constexpr int kBlock = 256;
constexpr size_t kLdsSceneBytes = 16 * 1024;   // LDS plan: 5-6 blocks/CU x (stack + scene) must fit 160 KiB
constexpr size_t kLdsOctBytes = 14 * 1024;     // ... with the octant node copies: 5 x (8 + 10 + 14) KiB
constexpr int kLdsMaxDepth = 16;                // LDS plan: binary stacks of 8 or 16 entries
// float4 slots of the octant plan's nodes in LDS (scene_to_lds): 8 x 3 per
// node for the boxes, then one int2 of child refs per node
__host__ __device__ constexpr int oct_lds_node_slots(int n_nodes) { return 24 * n_nodes + (n_nodes + 1) / 2; }
#ifndef FRT_QUEUE_GRAB
#define FRT_QUEUE_GRAB 64
#endif
constexpr int kQueueGrab = FRT_QUEUE_GRAB;      // path work queue: items a wave takes per atomic (at least)

struct DevWork {
    int nx, ny, spp, max_depth;
    uint32_t seed, s_off;                // frame seed, first global sample index (progressive passes)
    int tile, ntx, shard_index, shard_count;
    int spi, n_chunks;
    uint32_t n_items, n_slots;
    int trav_min;                        // shade when at most this many lanes of a wave still traverse
    int min_desc;                        // leaf postponing: see bvh2_step
    float *partial;                      // [n_chunks][n_slots][3]
    unsigned *counter;                   // work-queue head
    unsigned long long *wave_rays;       // [n_waves][4]: camera, extension, shadow, samples
    uint32_t grab;                       // items a wave takes per queue atomic (at least those it needs)
};

// slot -> pixel inside a tile: 8x8 blocks, row-major inside a block
__device__ __host__ __forceinline__ void slot_to_local(int s, int tile, int &lx, int &ly)
{
    const int b = s >> 6, l = s & 63;
    const int bpr = tile >> 3;
    lx = (b % bpr) * 8 + (l & 7);
    ly = (b / bpr) * 8 + (l >> 3);
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Small scenes (nodes + triangles + shading records + materials, <=
// kLdsSceneBytes) are copied into LDS once per block and traversed there
// (ds_read_b128 instead of L1/L2 round trips).  A wave's ds_read_b128 is
// served 16 lanes at a time from 64 banks: lanes reading distinct elements
// stay conflict-free when the elements' 16-B slots differ mod 16.  48-B
// records do that interleaved ((3 i + k) mod 16: triangles, the octant copies'
// node boxes), which puts every part at an immediate offset of one address;
// 64-B and 32-B records are copied planar (part k of element i at
// [k * count + i]), since interleaved only 4 or 8 slots would be used.
// Octant plan: 8 x n_nodes box records (3 float4), then the n_nodes child ref
// pairs (int2, one set for the 8 copies): 392 B per node instead of 512 B,
// 2 address VALU per node step instead of 5.
// HBM-resident scenes: the interleaved strides flatten_scene uses, as
// constants the compiler folds into the address arithmetic (kernel arguments
// would cost a quarter-rate v_mul_lo_u32 per node / triangle access).
__device__ __forceinline__ void scene_strides_hbm(DevScene &S)
{
    S.node_es = 4; S.node_ps = 1;
    S.node4_es = kNode4Parts; S.node4_ps = 1;
    S.tri_es = 3; S.tri_ps = 1;
    S.sh_es = 2; S.sh_ps = 1;
}

template <int WORLD>
__device__ __forceinline__ void scene_to_lds(DevScene &S, int *lds_base)
{
    // the LDS plans are binary (BVH4Q from LDS was 13 % slower on Cornell and was removed in round 4)
    static_assert(WORLD == FRT_WORLD_BVH || WORLD == kWorldBvh2Oct, "LDS plans hold a binary tree");
    constexpr bool OCT = WORLD == kWorldBvh2Oct;
    float4 *l4 = reinterpret_cast<float4 *>(lds_base);
    const DevScene S0 = S;
    const int nn = OCT ? oct_lds_node_slots(S0.n_nodes) : 4 * S0.n_nodes;
    const int nt = 3 * S0.n_tris, ns = 2 * S0.n_tris, nm = kMatStride * S0.n_mats;
    if constexpr (OCT) {   // node e = o * n_nodes + j, part k < 3 -> [3 e + k]; refs of j -> int2 [j]
        int2 *refs = reinterpret_cast<int2 *>(l4 + 24 * S0.n_nodes);
        for (int i = threadIdx.x; i < 32 * S0.n_nodes; i += kBlock) {
            const int e = i >> 2, k = i & 3;
            const float4 v = S0.nodes_oct[i];
            if (k < 3) l4[3 * e + k] = v;
            else if (e < S0.n_nodes) refs[e] = make_int2(f2i(v.x), f2i(v.y));
        }
        S.node_refs = refs;
    } else {
        for (int i = threadIdx.x; i < nn; i += kBlock) l4[(i & 3) * S0.n_nodes + (i >> 2)] = S0.nodes[i];
    }
    for (int i = threadIdx.x; i < nt; i += kBlock) l4[nn + i] = S0.tris[i];   // interleaved (48 B)
    for (int i = threadIdx.x; i < ns; i += kBlock) l4[nn + nt + (i & 1) * S0.n_tris + (i >> 1)] = S0.tshade[i];
    for (int i = threadIdx.x; i < nm; i += kBlock) l4[nn + nt + ns + i] = S0.mats[i];
    __syncthreads();
    S.nodes = l4;
    S.node_es = 1; S.node_ps = S0.n_nodes;
    S.tris = l4 + nn;
    S.tshade = l4 + nn + nt;
    S.mats = l4 + nn + nt + ns;
    S.tri_es = 3; S.tri_ps = 1;
    S.sh_es = 1; S.sh_ps = S0.n_tris;
}


// the octant node step of each integrator (bvh2_step's STEP): the path kernels
// store the far child without a branch (Cornell +0.4 %); AO and normals keep
// the branches (their rays agree more: Store cost AO 2.4 %, normals 3 %, same
// call, profiles/r05/r05af); PSS-MLT's chain kernel takes kStepSelect
#ifndef FRT_EXP_PATH_STEP
#define FRT_EXP_PATH_STEP kStepStore   // experiment builds vary the path kernels' form
#endif
#ifndef FRT_EXP_MLT_STEP
#define FRT_EXP_MLT_STEP kStepSelect   // ... and the chain kernel's
#endif
template <int KIND> constexpr int kPathStep = KIND == FRT_INTEGRATOR_PATH ? FRT_EXP_PATH_STEP : kStepBranch;
// ------------------------------------------------------------------------
// the persistent path megakernel
// ------------------------------------------------------------------------
// Work-item state of a lane: sample range, slot, chunk, pixel and the chunk's
// radiance sum, in an LDS column (kItemWords x kBlock ints after the traversal
// stack).  It is touched once per sample; as VGPRs it stayed live -- and
// spilled to scratch -- across every traversal and shading phase (spilled
// VGPRs at the register cap: cornell_1m 51 -> 24, Cornell 31 -> 6; same-call
// A/B +4.5 % / +1 %).
// (9 words -- the pixel index derived -- fit a 6th octant block per CU: 229.4 vs 229.1 ms at a
// 6-wave cap, 230.5 vs 230.2 at 5, profiles/r05/r05l; not kept)
// (7 words -- the end and the pixel coordinates derived -- measured 1 % slower on Cornell and
// +-0 on cornell_1m, also with the 4-wide plan's LDS stack grown to 15 entries: profiles/r06/r06i)
constexpr int kItemWords = 10;
enum { kIsCur, kIsEnd, kIsSlot, kIsChunk, kIsPix, kIsPx, kIsPy, kIsAcc };   // kIsAcc..+2: r, g, b
struct ItemState {
    int *b;      // the lane's column
    __device__ int get(int k) const { return b[k * kBlock]; }
    __device__ void set(int k, int x) const { b[k * kBlock] = x; }
};

// ---- the LDS footprint rule (host side) ----
// What scene_to_lds copies and the kernels lay out, in bytes, and whether it is within the budgets.
// Every place that asks "which plan does this scene get" -- the upload, the launch plans, the tree
// passes that append nodes, the self-tests -- asks here.
// rest: the float4s behind the nodes (triangles, shading records, materials)
constexpr size_t lds_planar_bytes(size_t n_nodes, size_t rest) { return sizeof(float4) * (4 * n_nodes + rest); }
constexpr size_t lds_octant_bytes(size_t n_nodes, size_t rest)
{
    return sizeof(float4) * (oct_lds_node_slots((int)n_nodes) + rest);
}
constexpr bool lds_planar_fits(size_t bytes) { return bytes <= kLdsSceneBytes; }
constexpr bool lds_octant_fits(size_t bytes) { return bytes <= kLdsOctBytes; }
// a block's LDS: the traversal stack (list worlds have none) and the item state of its lanes, then the scene
constexpr size_t lds_block_bytes(size_t stack, size_t scene_bytes, bool has_stack = true)
{
    return (has_stack ? stack * kBlock * sizeof(int) : 0) + (size_t)kItemWords * kBlock * sizeof(int) + scene_bytes;
}
// the rest of a FlatScene
template <class Scene> size_t lds_rest(const Scene &F) { return F.tris.size() + F.tshade.size() + F.mats.size(); }

// R: float (the product kernels) or double (the fp64 kernels, DESIGN.md
// "Precision": list worlds under FRT_PRECISION_AUTO, every plan under _FP64)
// sparse_kernel (frt_render_sparse.hip) holds a copy of this loop: a change here goes there too (DESIGN.md "One device loop")
template <int STACK, int WORLD, bool LDS_SCENE, int WAVES = 1, int MATS = kMatsNone,
          int KIND = FRT_INTEGRATOR_PATH, typename R = float>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WAVES))) void path_megakernel(
    const DevScene S0, const DevWork W)
{
    // [STACK][kBlock] stack, [kItemWords][kBlock] item state, then the scene
    extern __shared__ __attribute__((aligned(16))) int lds_mem[];
    int *stk = lds_mem + threadIdx.x;                                 // one LDS column per lane
    constexpr int kStackInts = WORLD != FRT_WORLD_LIST ? STACK * kBlock : 0;
    constexpr int kItemInts = kItemWords * kBlock;
    DevScene S = S0;
    if constexpr (LDS_SCENE) scene_to_lds<WORLD>(S, lds_mem + kStackInts + kItemInts);
    else scene_strides_hbm(S);
    const int lane = threadIdx.x & 63;
    const int T2 = W.tile * W.tile;

    // work-item state
    bool have_item = false, exhausted = false, active = false;
    // the wave's own item range [q_cur, q_end) from its last queue atomic (wave-uniform)
    uint32_t q_cur = 0, q_end = 0;
    const ItemState I{lds_mem + kStackInts + (int)threadIdx.x};
    PathState<R> P;
    // ray in flight: tracing = traversal steps remain; pending = finished, not yet shaded
    Trav<R> T;
    bool tracing = false, pending = false;
    int ovf[kOverflow<WORLD>];
    // ray counters are wave-uniform (SGPRs): popcounts of per-iteration ballots
    unsigned long long n_cam = 0, n_ext = 0, n_sh = 0, n_smp = 0;
    // HBM plans of the lambertian path kernels keep less per-lane state across
    // the traversal steps: the sample's radiance goes into the item's LDS sum
    // as it is found (NEE after a shadow ray, emission, environment), the RNG
    // key is re-derived from the item at shading, t_max from the ray kind.
    // cornell_1m +1.2 % (spilled VGPRs 26 -> 14); on the LDS plan it costs
    // 0.3 % (same-call A/B, profiles/r03/samecall/lean_*.jsonl).  The material
    // kernels keep the full state (DESIGN.md "Register-cap hazard"), and so do
    // the fp64 kernels (their per-sample sum stays fp64 until the sample ends).
    // The flushes round each contribution into the fp32 item sum, so a lean
    // plan's film equals the per-sample plans' to fp32 rounding, not bit for
    // bit (tests/test_gpu_parity.py::test_lean_plan_rounding).
    constexpr bool kLean = !LDS_SCENE && (MATS & ~kMatsFeatures) == kMatsNone && KIND == FRT_INTEGRATOR_PATH && !kIsF64<R>;
    auto flush_L = [&]() {
        I.set(kIsAcc + 0, f2i(i2f(I.get(kIsAcc + 0)) + (float)P.L.x));
        I.set(kIsAcc + 1, f2i(i2f(I.get(kIsAcc + 1)) + (float)P.L.y));
        I.set(kIsAcc + 2, f2i(i2f(I.get(kIsAcc + 2)) + (float)P.L.z));
        P.L = zero3<R>();
    };
    auto ray_tmax = [&]() -> R {
        if constexpr (kLean) return P.shadow ? R(1) - Cst<R>::shadow_eps : Cst<R>::tmax;
        else return P.rtmax;
    };

    // The lambertian path kernels of the LDS plans start an extension ray at its vertex's exit
    // root (host/exit_tree.cpp; the pass covers LDS-resident binary trees only).  Camera rays
    // (depth word 0) and shadow rays of either kind start where they did.
    constexpr bool kExit = LDS_SCENE && KIND == FRT_INTEGRATOR_PATH && (MATS & kMatsSpecAny) == 0 &&
                           (WORLD == FRT_WORLD_BVH || WORLD == kWorldBvh2Oct);

    unsigned long long diag_t0 = FRT_DIAG_CLOCK();
    for (;;) {
        FRT_DIAG_TICK(6);
        // ---- traversal: steps (descend to a leaf, test it) of every lane's ray,
        // until at most trav_min lanes are still traversing.  Lanes whose ray is
        // done wait here only while the rest of the wave needs few more steps;
        // then they shade together while the stragglers keep their state.
        for (;;) {
            bool shadow_done = false;
            if (tracing) FRT_DIAG_TICK(3);
            // (LDS-resident binary plans: no leaf postponing, compiled out)
            if (tracing && trav_step_world<WORLD, kBlock, STACK, kPathStep<KIND>>(T, S, P.ro, P.rd, P.shadow, stk, ovf,
                                                                       LDS_SCENE && (WORLD == FRT_WORLD_BVH || WORLD == kWorldBvh2Oct)
                                                                           ? 0 : W.min_desc)) {
                if (KIND == FRT_INTEGRATOR_PATH && P.shadow) {   // finish the shadow ray here, keep traversing
                    if (path_after_shadow<MATS>(P, T.h.prim < 0)) {
                        if constexpr (kLean) flush_L();
                        shadow_done = true;
                        if constexpr (kExit) {
                            const int xr = exit_root(P);
                            tracing = trav_begin(T, S, xr ? xr : S.root, P.ro, P.rd, ray_tmax());
                        } else {
                            tracing = trav_begin_world<WORLD>(T, S, P.ro, P.rd, ray_tmax());
                        }
                        pending = !tracing;
                    } else {                                      // path ended (P.term): shade finishes it
                        tracing = false;
                        pending = true;
                    }
                } else {
                    tracing = false;
                    pending = true;
                }
            }
            n_ext += __popcll(__ballot(shadow_done));
            if (__popcll(__ballot(tracing)) <= W.trav_min) break;
        }
        // ---- shade the finished rays ----
        const unsigned long long diag_t1 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(16, diag_t1 - diag_t0);
        uint32_t ne = 0, ns = 0;
        bool next_ray = false;
        if (pending) {
            FRT_DIAG_TICK(4);
            pending = false;
            if constexpr (kLean)
                P.key = smp_key<MATS>(W.seed, (uint32_t)I.get(kIsPix), (uint32_t)(I.get(kIsCur) - 1) + W.s_off);
            const bool done = shade_kind<KIND, MATS, kExit>(P, S, T.h, W.max_depth, ne, ns);
            if (done || kLean) flush_L();   // fp32 chunk sums in either precision
            active = !done;
            next_ray = !done;
        }
        n_ext += __popcll(__ballot(ne != 0));
        n_sh += __popcll(__ballot(ns != 0));
        const unsigned long long diag_t2 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(17, diag_t2 - diag_t1);
        // ---- retire a finished item: its chunk sum goes to its own slot ----
        if (!active && have_item && I.get(kIsCur) >= I.get(kIsEnd)) {
            float *dst = W.partial + 3ull * ((size_t)(uint32_t)I.get(kIsChunk) * W.n_slots + (uint32_t)I.get(kIsSlot));
            dst[0] = i2f(I.get(kIsAcc + 0)); dst[1] = i2f(I.get(kIsAcc + 1)); dst[2] = i2f(I.get(kIsAcc + 2));
            have_item = false;
        }
        // ---- wave-aggregated refill, lanes ranked by mbcnt: items come from the
        // wave's own range first; when it runs short, one atomic takes
        // max(grab, still needed) more.  With one atomic per refill every wave
        // of the grid queued on one counter: AO (1.5 rays a sample) took 72.5 ms
        // at 1080p 512 spp, 31.9 ms with 64 items a grab; Cornell path +1.0 %,
        // cornell_1m +1.6 %; 256 a grab lengthens the frame's tail
        // (profiles/r03/samecall/grab_*.jsonl).  Items are disjoint and each
        // (chunk, slot) sum has one writer, so the film does not depend on it. ----
        const bool need = !active && !have_item && !exhausted;
        const uint64_t m = __ballot(need);
        if (m) {
            const uint32_t nm = (uint32_t)__popcll(m), r = lane_rank(m);
            const uint32_t left = q_end - q_cur;
            uint32_t w;
            if (nm <= left) {
                w = q_cur + r;
                q_cur += nm;
            } else {
                const uint32_t take = max(W.grab, nm - left);
                const int leader = __ffsll((unsigned long long)m) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(W.counter, take);
                base = __shfl(base, leader);
                w = r < left ? q_cur + r : base + (r - left);
                q_cur = base + (nm - left);
                q_end = base + take;
            }
            if (need) {
                if (w >= W.n_items) {
                    exhausted = true;
                } else {
                    const uint32_t s = w % (uint32_t)T2;
                    const uint32_t q = w / (uint32_t)T2;
                    const uint32_t chunk = q % (uint32_t)W.n_chunks;
                    const uint32_t t_ord = q / (uint32_t)W.n_chunks;
                    const int tile_id = W.shard_index + (int)t_ord * W.shard_count;
                    int lx, ly;
                    slot_to_local((int)s, W.tile, lx, ly);
                    const int px = (tile_id % W.ntx) * W.tile + lx;
                    const int py = (tile_id / W.ntx) * W.tile + ly;
                    if (px < W.nx && py < W.ny) {   // padding slots of edge tiles carry no work
                        have_item = true;
                        const int s_cur = (int)chunk * W.spi;
                        I.set(kIsCur, s_cur);
                        I.set(kIsSlot, (int)(t_ord * (uint32_t)T2 + s));
                        I.set(kIsChunk, (int)chunk);
                        I.set(kIsPix, py * W.nx + px);
                        I.set(kIsEnd, min(W.spp, s_cur + W.spi));
                        I.set(kIsPx, px);
                        I.set(kIsPy, py);
                        I.set(kIsAcc + 0, 0); I.set(kIsAcc + 1, 0); I.set(kIsAcc + 2, 0);
                    }
                }
            }
        }
        // ---- next camera sample of the item ----
        const bool start = !active && have_item && I.get(kIsCur) < I.get(kIsEnd);
        if (start) {
            const int s_cur = I.get(kIsCur);
            path_begin<MATS>(P, S, I.get(kIsPx), I.get(kIsPy), W.nx, W.ny, W.seed, (uint32_t)I.get(kIsPix),
                       (uint32_t)s_cur + W.s_off);
            I.set(kIsCur, s_cur + 1);
            active = true;
            next_ray = true;
        }
        const unsigned long long started = __popcll(__ballot(start));
        n_cam += started;
        n_smp += started;
        // ---- set up the next ray's traversal (a scene miss is finished at once) ----
        if (next_ray) {
            // an area-light shadow ray starts at the shadow root (the environment-NEE ray has t_max = tmax)
            const R tm = ray_tmax();
            const bool occl = KIND == FRT_INTEGRATOR_PATH && P.shadow && ((MATS & kMatsEnvNee) == 0 || tm < R(1));
            if constexpr (kExit) {
                const int xr = P.shadow ? 0 : exit_root(P);
                tracing = trav_begin(T, S, xr ? xr : S.root, P.ro, P.rd, tm, occl);
            } else {
                tracing = trav_begin_world<WORLD>(T, S, P.ro, P.rd, tm, occl);
            }
            pending = !tracing;
        }
        diag_t0 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(18, diag_t0 - diag_t2);
        if (__ballot(active || !exhausted) == 0) break;
    }
    // per-wave ray counters, no atomics: lane 0 writes the wave's sums
    const unsigned long long c[4] = {n_cam, n_ext, n_sh, n_smp};
    if (lane == 0) {
        const size_t wv = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
        for (int k = 0; k < 4; ++k) W.wave_rays[4 * wv + k] = c[k];
    }
}


// ------------------------------------------------------------------------
// ray queries (frt_trace_device): a buffer of rays through the same
// resumable traversal, Scene::world->hit (path.cpp:10, 50; parallel_bvh.h:39-64,
// hitable_list.cpp:4-21) batched.  Persistent; a lane whose ray is done takes
// the next ray at once, so the wave's lanes stay busy until the buffer runs
// dry.  Rays come from a wave-local chunk (kTraceChunk rays taken with one
// atomic); a global atomic per refill put its latency on every traversal
// step (4 Grays/s on camera rays: profiles/r03/r03e_trace_atomic_per_step.jsonl).
// ------------------------------------------------------------------------
constexpr uint32_t kTraceChunk = 256;   // rays a wave takes from the buffer with one atomic
// the context's queue words: [0] the render / PSS-MLT work queue, [kTraceCounterWord] the ray-query queue
constexpr size_t kCounterBytes = 256;
constexpr int kTraceCounterWord = 32;   // 128 B after the render queue's word
struct DevRays {
    const float4 *ray;       // 2 per ray: (origin, t_max) | (direction, flags: bit 0 = any-hit)
    float4 *hit;             // 1 per ray: (t, u, v, prim ref of the scene view as int bits; -1 = miss)
    uint32_t n;
    int min_desc;            // leaf postponing (bvh2_step)
    unsigned *counter;       // ray-queue head
};
template <int STACK, int WORLD, bool LDS_SCENE, int WAVES>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WAVES))) void trace_kernel(
    const DevScene S0, const DevRays R)
{
    extern __shared__ __attribute__((aligned(16))) int lds_mem[];
    int *stk = lds_mem + threadIdx.x;                                 // one LDS column per lane
    constexpr int kStackInts = WORLD != FRT_WORLD_LIST ? STACK * kBlock : 0;
    DevScene S = S0;
    if constexpr (LDS_SCENE) scene_to_lds<WORLD>(S, lds_mem + kStackInts);
    else scene_strides_hbm(S);
    const int lane = threadIdx.x & 63;
    Trav<float> T;
    int ovf[kOverflow<WORLD>];
    f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
    bool anyhit = false, tracing = false, exhausted = false;
    uint32_t id = 0;
    auto finish = [&]() {
        const int p = T.h.prim;
        const int ref = (p < 0 || (p & FRT_PRIM_SPHERE)) ? p : S.tri_view[p];
        R.hit[id] = make_float4(T.h.t, T.h.u, T.h.v, i2f(ref));
    };
    // Each lane holds the NEXT ray of its queue in registers (loaded while the
    // current one traverses), so a lane that finishes starts its next ray
    // without waiting on memory.
    uint32_t chunk_next = 0, chunk_end = 0;                          // wave-uniform
    float4 na = make_float4(0, 0, 0, 0), nb = make_float4(0, 0, 0, 0);
    uint32_t nid = 0;
    bool have_next = false;
    for (;;) {
        if (!tracing && have_next) {                                  // start the prefetched ray
            id = nid;
            o = xyz(na);
            d = xyz(nb);
            anyhit = (f2i(nb.w) & 1) != 0;
            have_next = false;
            tracing = trav_begin_world<WORLD>(T, S, o, d, na.w);
            if (!tracing) finish();                                   // the ray misses the scene box
        }
        const bool need = !have_next && !exhausted;
        const uint64_t m = __ballot(need);
        if (m) {
            // the wave's lanes without a queued ray take the rest of its chunk,
            // then a new chunk (one atomic per kTraceChunk rays) once it runs short
            const uint32_t want = (uint32_t)__popcll(m), left = chunk_end - chunk_next;
            uint32_t fresh = 0xffffffffu;
            if (left < want && chunk_end < R.n) {
                uint32_t b0 = 0;
                if (lane == 0) b0 = atomicAdd(R.counter, kTraceChunk);
                fresh = __builtin_amdgcn_readfirstlane(__shfl(b0, 0));
            }
            const uint32_t rank = lane_rank(m);
            const uint32_t w = rank < left ? chunk_next + rank : (fresh == 0xffffffffu ? 0xffffffffu : fresh + (rank - left));
            if (left >= want) {
                chunk_next += want;
            } else if (fresh != 0xffffffffu) {
                chunk_next = fresh + (want - left);
                chunk_end = fresh + kTraceChunk;
            } else {
                chunk_next = chunk_end;
            }
            if (need) {
                if (w >= R.n) {
                    exhausted = true;
                } else {
                    nid = w;
                    na = R.ray[2 * (size_t)w];
                    nb = R.ray[2 * (size_t)w + 1];
                    have_next = true;
                }
            }
        }
        if (__ballot(tracing || have_next) == 0) break;
        if (tracing && trav_step_world<WORLD, kBlock, STACK>(T, S, o, d, anyhit, stk, ovf,
                                                             LDS_SCENE && (WORLD == FRT_WORLD_BVH || WORLD == kWorldBvh2Oct) ? 0 : R.min_desc)) {
            tracing = false;
            finish();
        }
    }
}

// ------------------------------------------------------------------------
// PSS-MLT (pssmlt.cpp:301-365)
// ------------------------------------------------------------------------
// chain state columns (ItemState over kChainWords words): step count, chain
// index, the current state's film position, scalar contribution, pending
// weight and colour
constexpr int kChainWords = 9;
enum { kCsT, kCsC, kCsX, kCsY, kCsSc, kCsW, kCsCc };   // kCsCc..+2: r, g, b
struct MltWork {
    int nx, ny;
    uint32_t seed;
    int shard_index, shard_count;
    uint32_t n_local;                    // chains of this shard: global c = shard_index + j * shard_count
    uint64_t steps;                      // mutations per chain
    float b, scale, s2p, logp;           // normaliser, nx*ny/ns, pixel-dim perturb constants
    int trav_min;                        // see path_megakernel / trav_min()
    int min_desc;                        // leaf postponing: see bvh2_step
    float *U;                            // [n_local][kMltRow] current primary samples + fingerprint (frt_mlt.hpp)
    unsigned long long *film;            // [nx*ny*3] splat accumulation, fixed point (kSplatFix)
    unsigned *counter;
    unsigned long long *wave_rays;
};

template <int WORLD, int STACK>
__device__ __forceinline__ Hit<float> trace_any(const DevScene &S, const PathState<float> &P, int *stk)
{
    return trace<WORLD, kBlock, STACK>(S, P.ro, P.rd, P.rtmax, P.shadow, stk, P.shadow);   // pssmlt::Li: every shadow ray ends on a light
}

// bootstrap: sc of n_init independent eye paths (pssmlt.cpp:303-312); the host
// sums them in a fixed order
template <int STACK, int WORLD, bool MATS, bool ENV = false>
__global__ __launch_bounds__(kBlock) void mlt_bootstrap(const DevScene S0, int nx, int ny, uint32_t seed, int n_init,
                                                        float *sc)
{
    DevScene S = S0;
    scene_strides_hbm(S);
    extern __shared__ __attribute__((aligned(16))) int lds_mem[];
    int *stk = lds_mem + threadIdx.x;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_init) return;
    PrndSource src{nullptr, 0, 0, rng_key(seed ^ kMltBootSalt, (uint32_t)i, 0u), 0u, true, 0.0f, 0.0f};
    MltPath M;
    mlt_begin(M, S, src, nx, ny);
    uint32_t ne = 0, ns = 0;
    for (;;) {
        if (mlt_beyond(M)) { M.P.L = M.P.L + M.P.beta * env_radiance<(ENV ? kMatsEnv : kMatsNone)>(S, M.P.rd); break; }
        const Hit<float> h = trace_any<WORLD, STACK>(S, M.P, stk);
        if (mlt_shade<MATS, ENV>(M, S, h, src, ne, ns)) break;
    }
    sc[i] = fmaxf(fmaxf(M.P.L.x, M.P.L.y), M.P.L.z);
}

// Splats (AccumulatePathContribution, pssmlt.cpp) add into a fixed-point film:
// a splat is rounded to a multiple of 2^-kSplatFix and added with a 64-bit
// integer atomic.  Integer sums do not depend on the order the chains' atomics
// land in, so the film is bit-reproducible run to run (float atomics were
// not).  Splats are >= 0 (scale, weights and radiance are); the quantum
// 2^-36 = 1.5e-11 is far below fp32's resolution of the pixel values, and a
// signed 64-bit pixel holds up to 2^27 before it wraps.  A splat that is not a
// finite value in [0, 2^27) is dropped (the reference's pixel would turn NaN /
// Inf there; none occurs in the test scenes).  mlt_film_to_float converts once
// at the end.
constexpr int kSplatFix = 36;
__device__ __forceinline__ void mlt_splat(const MltWork &W, float x, float y, f3 c, float w)
{
    const int pix = mlt_pixel(x, y, W.nx, W.ny);
    if (pix < 0) return;
    const float k = W.scale * w;
    const double q = (double)(1ull << kSplatFix), lim = 9.2233720368547758e18;   // 2^63
    const double v[3] = {(double)(k * c.x) * q, (double)(k * c.y) * q, (double)(k * c.z) * q};
    if (!(v[0] >= 0.0 && v[0] < lim && v[1] >= 0.0 && v[1] < lim && v[2] >= 0.0 && v[2] < lim)) return;
    unsigned long long *f = W.film + 3 * (size_t)pix;
    atomicAdd(f + 0, (unsigned long long)__double2ll_rn(v[0]));
    atomicAdd(f + 1, (unsigned long long)__double2ll_rn(v[1]));
    atomicAdd(f + 2, (unsigned long long)__double2ll_rn(v[2]));
}

// one lane = one chain tracing the rays of its current eye path (initial
// state, then one proposal per mutation); traversal steps interleave with
// shading as in path_megakernel
#ifndef FRT_EXP_MLT_WAVES
#define FRT_EXP_MLT_WAVES 4      // register cap of the chain kernel: 4 waves/SIMD.  Round 1 measured 5
#endif                           // +17 % over the compiler's own allocation (profiles/r01_expmlt1.txt);
                                 // round 4's kernel: 4 waves 690.8 ms, 5 waves 700.5, 6 waves 783.9
                                 // (same call, profiles/r04/r04g); experiment builds vary it
template <int STACK, int WORLD, bool LDS_SCENE, bool MATS, bool ENV = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(FRT_EXP_MLT_WAVES))) void mlt_megakernel(
    const DevScene S0, const MltWork W)
{
    // [STACK][kBlock] stack, [kChainWords][kBlock] chain state, then the scene
    extern __shared__ __attribute__((aligned(16))) int lds_mem[];
    int *stk = lds_mem + threadIdx.x;
    constexpr int kStackInts = WORLD != FRT_WORLD_LIST ? STACK * kBlock : 0;
    DevScene S = S0;
    if constexpr (LDS_SCENE) scene_to_lds<WORLD>(S, lds_mem + kStackInts + kChainWords * kBlock);
    else scene_strides_hbm(S);
    const int lane = threadIdx.x & 63;
    bool have = false, exhausted = false, init = false, large = false;
    // the chain's current state (touched once per proposal) in an LDS column,
    // as the path kernel's work item (ItemState)
    const ItemState C{lds_mem + kStackInts + (int)threadIdx.x};
    uint32_t j = 0;
    RngKey key{0, 0};
    MltPath M;
    uint32_t n_cam = 0, n_ext = 0, n_sh = 0, n_smp = 0;

    auto source = [&]() {
        PrndSource src{W.U, W.n_local, j, key, 2u, init || large, W.s2p, W.logp};
        return src;
    };
    // ray in flight, as in path_megakernel: tracing = traversal steps remain;
    // pending = finished (or the path went beyond MaxPathLength), not yet shaded
    Trav<float> T;
    bool tracing = false, pending = false, beyond = false;
    int ovf[kOverflow<WORLD>];
    // diagnostic build (FRT_DIAG, tools/diag_phases.py --integrator pssmlt): lane
    // counts of the traversal (pairs 1, 2, 7 in bvh2_step), step loop (3),
    // shading (4), accept / reject (5), outer loop (6); cycles of the step loop
    // (16), shading (17), accept / reject + splats (19), row materialisation
    // (20), queue + next proposal (18)
    unsigned long long diag_t0 = FRT_DIAG_CLOCK();
    for (;;) {
        FRT_DIAG_TICK(6);
        // ---- traversal steps until at most trav_min lanes still traverse ----
        for (;;) {
            bool ext = false;
            if (tracing) FRT_DIAG_TICK(3);
            if (tracing && trav_step_world<WORLD, kBlock, STACK, FRT_EXP_MLT_STEP>(T, S, M.P.ro, M.P.rd, M.P.shadow, stk, ovf,
                                                                 LDS_SCENE ? 0 : W.min_desc)) {   // LDS plans: compiled out
                if (M.P.shadow) {               // finish the shadow ray here (mlt_shade's shadow branch)
                    if (!path_after_shadow<(MATS ? kMatsAll : kMatsNone)>(M.P, T.h.prim < 0)) {   // path ended (P.term)
                        tracing = false;
                        pending = true;
                    } else if (mlt_beyond(M)) {
                        beyond = true;
                        tracing = false;
                        pending = true;
                    } else {
                        ext = true;
                        tracing = trav_begin_world<WORLD>(T, S, M.P.ro, M.P.rd, M.P.rtmax, M.P.shadow);
                        pending = !tracing;
                    }
                } else {
                    tracing = false;
                    pending = true;
                }
            }
            if (ext) ++n_ext;                   // per-lane counters, reduced at the end
            if (__popcll(__ballot(tracing)) <= W.trav_min) break;
        }
        bool next_ray = false, done = false;
        const unsigned long long diag_t1 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(16, diag_t1 - diag_t0);
        if (pending) {
            FRT_DIAG_TICK(4);
            pending = false;
            if (beyond) {                               // pssmlt.cpp:151, :276
                M.P.L = M.P.L + M.P.beta * env_radiance<(ENV ? kMatsEnv : kMatsNone)>(S, M.P.rd);
                beyond = false;
                done = true;
            } else {
                uint32_t ne = 0, ns = 0;
                done = mlt_shade<MATS, ENV>(M, S, T.h, source(), ne, ns);
                n_ext += ne; n_sh += ns;
                next_ray = !done;
            }
        }
        // accept / reject (per lane); the accepted proposal's row is written below
        const unsigned long long diag_t2 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(17, diag_t2 - diag_t1);
        bool mat = false, mat_fresh = false, setup_next = false;
        RngKey mat_key = key;
        if (done) {
            FRT_DIAG_TICK(5);
            const f3 L = M.P.L;
            const float sc = fmaxf(fmaxf(L.x, L.y), L.z);
            float cx = i2f(C.get(kCsX)), cy = i2f(C.get(kCsY)), csc = i2f(C.get(kCsSc)), cw = i2f(C.get(kCsW));
            f3 cc = mk3(i2f(C.get(kCsCc)), i2f(C.get(kCsCc + 1)), i2f(C.get(kCsCc + 2)));
            uint32_t t = (uint32_t)C.get(kCsT);
            bool moved = false;
            if (init) {                                 // current = initial state, materialised
                mat = true; mat_fresh = true;
                cx = M.x; cy = M.y; cc = L; csc = sc;
                moved = true;
                init = false;
            } else {                                    // pssmlt.cpp:200-209
                float a = 1.0f;
                if (csc > 0.0f) a = fmaxf(fminf(1.0f, sc / csc), 0.0f);
                if (sc > 0.0f) mlt_splat(W, M.x, M.y, L, (a + (large ? 1.0f : 0.0f)) / (sc / W.b + kMltLargeStep));
                if (csc > 0.0f) cw += (1.0f - a) / (csc / W.b + kMltLargeStep);
                if (rng_u(key, 1) <= a) {               // accept: splat the old state's weight, move
                    if (csc > 0.0f && cw != 0.0f) mlt_splat(W, cx, cy, cc, cw);
                    uint2 *fp = reinterpret_cast<uint2 *>(W.U + (size_t)j * kMltRow + kMltFp);
                    uint2 f = *fp;                      // trajectory fingerprint: (accepts, sum of 1-based steps)
                    f.x += 1u; f.y += t + 1u;
                    *fp = f;
                    cw = 0.0f;
                    mat = true; mat_fresh = large;
                    cx = M.x; cy = M.y; cc = L; csc = sc;
                    moved = true;
                }
                ++t;
                ++n_smp;
            }
            if ((uint64_t)t >= W.steps) {               // chain finished
                if (csc > 0.0f && cw != 0.0f) mlt_splat(W, cx, cy, cc, cw);
                have = false;
            } else {
                setup_next = true;
                C.set(kCsT, (int)t);
                C.set(kCsW, f2i(cw));
                if (moved) {
                    C.set(kCsX, f2i(cx)); C.set(kCsY, f2i(cy)); C.set(kCsSc, f2i(csc));
                    C.set(kCsCc, f2i(cc.x)); C.set(kCsCc + 1, f2i(cc.y)); C.set(kCsCc + 2, f2i(cc.z));
                }
            }
        }
        // ---- materialise accepted proposals: the rows of the wave's n accepted
        // chains as one flat range of n * 92 elements over the 64 lanes
        // (element e: chain rank e / 92, dimension e % 92).  A ds_permute first
        // moves the r-th accepted chain's (row, key, fresh) to lane r (the other
        // lanes fill lanes n..63, so it is a permutation).  Coalesced along each
        // row; only the last trip has idle lanes (one chain at a time left 28 of
        // 64 lanes idle on every second trip).  The whole wave is active here. ----
        const unsigned long long diag_t3 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(19, diag_t3 - diag_t2);
        if (const uint64_t mm = __ballot(mat)) {
            const uint32_t n = (uint32_t)__popcll(mm);
            const int dst = 4 * (int)(mat ? lane_rank(mm) : n + lane_rank(~mm));   // byte address of the target lane
            const uint32_t rj = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(j | (mat_fresh ? 0x80000000u : 0u)));
            const uint32_t rk0 = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)mat_key.k0);
            const uint32_t rk1 = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)mat_key.k1);
            const uint32_t total = n * (uint32_t)kMltDims;
            for (uint32_t e0 = 0; e0 < total; e0 += 64) {
                const uint32_t e = e0 + (uint32_t)lane;
                const uint32_t r = min(e / (uint32_t)kMltDims, n - 1u);
                const uint32_t jl = (uint32_t)__shfl((int)rj, (int)r);   // every lane active: sources are lanes < n
                const RngKey kl{(uint32_t)__shfl((int)rk0, (int)r), (uint32_t)__shfl((int)rk1, (int)r)};
                if (e < total) {
                    const int d = (int)(e - r * (uint32_t)kMltDims);
                    float *row = W.U + (size_t)(jl & 0x7fffffffu) * kMltRow;   // j < 2^31: bit 31 = fresh
                    const float u = rng_u(kl, 2u + (uint32_t)d);
                    row[d] = (jl >> 31) ? u : mlt_mutate(row[d], u, d, W.s2p, W.logp);
                }
            }
        }
        const unsigned long long diag_t4 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(20, diag_t4 - diag_t3);
        if (setup_next) {                               // next proposal reads the new state
            key = rng_key(W.seed ^ kMltChainSalt, (uint32_t)C.get(kCsC), (uint32_t)C.get(kCsT) + 1u);
            large = rng_u(key, 0) < kMltLargeStep;      // large_step vs mutate (pssmlt.cpp:187-196)
            mlt_begin(M, S, source(), W.nx, W.ny);
            ++n_cam;
            next_ray = true;
        }
        // ---- chains from the queue, one atomic per wave ----
        const bool need = !have && !exhausted;
        const uint64_t m = __ballot(need);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(W.counter, (unsigned)__popcll(m));
            base = __shfl(base, leader);
            if (need) {
                const uint32_t w = base + lane_rank(m);
                if (w >= W.n_local) {
                    exhausted = true;
                } else {
                    have = true;
                    init = true;
                    j = w;
                    *reinterpret_cast<uint2 *>(W.U + (size_t)w * kMltRow + kMltFp) = make_uint2(0u, 0u);
                    const uint32_t c = (uint32_t)W.shard_index + w * (uint32_t)W.shard_count;
                    C.set(kCsC, (int)c);
                    C.set(kCsT, 0);
                    C.set(kCsW, 0);
                    C.set(kCsSc, 0);
                    key = rng_key(W.seed ^ kMltChainSalt, c, 0u);   // initial state: TMarkovChain(s)
                    mlt_begin(M, S, source(), W.nx, W.ny);
                    ++n_cam;
                    next_ray = true;
                }
            }
        }
        // ---- next ray of the eye path ----
        if (next_ray) {
            if (mlt_beyond(M)) {
                beyond = true;
                pending = true;
            } else {
                tracing = trav_begin_world<WORLD>(T, S, M.P.ro, M.P.rd, M.P.rtmax, M.P.shadow);
                pending = !tracing;
            }
        }
        diag_t0 = FRT_DIAG_CLOCK();
        FRT_DIAG_CYC(18, diag_t0 - diag_t4);
        if (__ballot(have || !exhausted) == 0) break;
    }
    unsigned long long cnt[4] = {n_cam, n_ext, n_sh, n_smp};
    for (int k = 0; k < 4; ++k)
        for (int off = 32; off > 0; off >>= 1) cnt[k] += __shfl_xor(cnt[k], off);
    if (lane == 0) {
        const size_t wv = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
        for (int k = 0; k < 4; ++k) W.wave_rays[4 * wv + k] = cnt[k];
    }
}

}  // namespace
