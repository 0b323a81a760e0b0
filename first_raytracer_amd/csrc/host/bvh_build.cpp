// bvh_build.cpp -- parallel_bvh_node::create_bvh (parallel_bvh.h:67-175): the
// SAH split rule with glibc's merge-sort qsort order (bvh.h:6-55 comparators),
// built with std::thread subtrees instead of taskflow subflows; and the binned
// SAH builder behind frt_scene_build_bvh_sah.
#include "bvh_build.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <exception>
#include <thread>
#include <utility>

#include "frt.h"

namespace frt_bvh {

std::vector<Box> prim_boxes(const double *tri_v, const double *sphere, const int32_t *refs, size_t n)
{
    std::vector<Box> boxes(n);
    for (size_t i = 0; i < n; ++i) {
        const int ref = refs[i];
        Box &b = boxes[i];
        if (ref & FRT_PRIM_SPHERE) {
            const double *sp = &sphere[4 * (size_t)(ref & ~FRT_PRIM_SPHERE)];
            for (int k = 0; k < 3; ++k) { b.lo[k] = sp[k] - sp[3]; b.hi[k] = sp[k] + sp[3]; }
        } else {
            const double *v = &tri_v[9 * (size_t)ref];
            for (int k = 0; k < 3; ++k) {  // triangle.h:120-137
                b.lo[k] = std::fmin(std::fmin(v[k], v[3 + k]), v[6 + k]);
                b.hi[k] = std::fmax(std::fmax(v[k], v[3 + k]), v[6 + k]);
            }
        }
    }
    return boxes;
}

int tree_depth(const std::vector<int32_t> &node_child, int32_t root)
{
    const size_t n_nodes = node_child.size() / 2;
    if (root < 0 || n_nodes == 0) return 0;
    int depth = 0;
    size_t visited = 0;
    std::vector<std::pair<int32_t, int>> st{{root, 1}};
    while (!st.empty()) {
        const auto [node, d] = st.back();
        st.pop_back();
        if ((size_t)node >= n_nodes || ++visited > n_nodes) return -1;
        depth = std::max(depth, d);
        for (int side = 0; side < 2; ++side)
            if (node_child[2 * (size_t)node + side] >= 0) st.push_back({node_child[2 * (size_t)node + side], d + 1});
    }
    return depth;
}

namespace {

// what both builders fill: the arrays of a Tree, nodes numbered as they are begun
struct Nodes {
    std::vector<double> box;
    std::vector<int32_t> child;
    std::atomic<int> count{0};

    explicit Nodes(size_t n_prims) : box(6 * (n_prims - 1), 0.0), child(2 * (n_prims - 1), 0) {}

    // Node `me` (= count.fetch_add(1) when its builder began it) over n prims at
    // level `depth`: its two sides, each a leaf ~slot or a subtree's root that
    // reports its levels; large subtrees on their own thread (taskflow subflows
    // in the reference).  levels: those of interior nodes below and with this one
    // (what tree_depth counts, without a pass over a million nodes).
    template <class L, class R>
    int32_t close(int me, const Box &b, int n, int depth, int &levels, L left, R right)
    {
        int32_t l = 0, r = 0;
        int ll = 0, lr = 0;
        if (n > 65536 && depth < 6) {
            std::exception_ptr thrown;
            std::thread th([&] {
                try { l = left(ll); } catch (...) { thrown = std::current_exception(); }
            });
            try { r = right(lr); } catch (...) { th.join(); throw; }
            th.join();
            if (thrown) std::rethrow_exception(thrown);
        } else {
            l = left(ll);
            r = right(lr);
        }
        for (int k = 0; k < 3; ++k) { box[6 * (size_t)me + k] = b.lo[k]; box[6 * (size_t)me + 3 + k] = b.hi[k]; }
        child[2 * (size_t)me] = l;
        child[2 * (size_t)me + 1] = r;
        levels = 1 + std::max(ll, lr);
        return me;
    }
};

// ---------------------------------------------------------------------------
// parallel_bvh_node construction (parallel_bvh.h:67-160)
// ---------------------------------------------------------------------------
struct Sweep {
    const Box *B;   // per slot
    Nodes out;

    // glibc msort_with_tmp (stdlib/msort.c) with the bvh.h comparator:
    // cmp(a,b) = (key[a] - key[b] < 0) ? -1 : 1; "<= 0" takes from the left run.
    static void msort(int32_t *b, size_t n, int32_t *tmp, const Box *boxes, int axis)
    {
        if (n <= 1) return;
        const size_t n1 = n / 2, n2 = n - n1;
        int32_t *b1 = b, *b2 = b + n1;
        msort(b1, n1, tmp, boxes, axis);
        msort(b2, n2, tmp, boxes, axis);
        size_t i = n1, j = n2;
        int32_t *t = tmp;
        while (i > 0 && j > 0) {
            if (boxes[*b1].lo[axis] - boxes[*b2].lo[axis] < 0.0) { *t++ = *b1++; --i; }
            else { *t++ = *b2++; --j; }
        }
        if (i > 0) memcpy(t, b1, i * sizeof(int32_t));
        memcpy(b, tmp, (n - j) * sizeof(int32_t));
    }

    // node over the slots l[0, n)
    int32_t build(int32_t *l, int n, int depth, int &levels)
    {
        const int me = out.count.fetch_add(1);
        Box main_box = B[l[0]];
        for (int i = 1; i < n; ++i) main_box = surround(B[l[i]], main_box);
        const int axis = longest_axis(main_box);
        int idx = 0;
        {
            std::vector<int32_t> tmp(n);
            msort(l, (size_t)n, tmp.data(), B, axis);
            std::vector<double> left_area(n), right_area(n);
            left_area[0] = box_area(B[l[0]]);
            Box lb = B[l[0]];
            for (int i = 1; i < n - 1; ++i) { lb = surround(lb, B[l[i]]); left_area[i] = box_area(lb); }
            right_area[n - 1] = box_area(B[l[n - 1]]);
            Box rb = B[l[n - 1]];
            for (int i = n - 2; i > 0; --i) { rb = surround(rb, B[l[i]]); right_area[i] = box_area(rb); }
            double min_sah = 3.40282346638528859812e+38;  // FLT_MAX
            for (int i = 0; i < n - 1; ++i) {
                const double sah = i * left_area[i] + (n - i - 1) * right_area[i + 1];
                if (sah < min_sah) { idx = i; min_sah = sah; }
            }
        }   // (the scratch arrays are gone before the recursion)
        return out.close(
            me, main_box, n, depth, levels, [&](int &lv) { return (idx == 0) ? ~l[0] : build(l, idx + 1, depth + 1, lv); },
            [&](int &lv) { return (idx == n - 2) ? ~l[idx + 1] : build(l + idx + 1, n - idx - 1, depth + 1, lv); });
    }
};

// ---------------------------------------------------------------------------
// Binned SAH builder (frt_scene_build_bvh_sah): 32 centroid bins on each axis,
// cost N_L A_L + N_R A_R, single-primitive leaves (the upload collapses
// subtrees of <= 4 triangles).  A higher-quality tree than both the
// reference's sweep (sorted by box minimum) and the GPU LBVH, at host cost.
// ---------------------------------------------------------------------------
// centroid bins per axis: 32 (8-128 measured 1-2 % apart on the GPU,
// profiles/r01d_ab_sah_bins.txt).  A build-time constant, so no stray
// environment can change the tree (and with it which of two exactly tied
// hits a ray reports); experiment builds set FRT_EXP_SAH_BINS.
#ifndef FRT_EXP_SAH_BINS
#define FRT_EXP_SAH_BINS 32
#endif
struct Binned {
    static constexpr int kBins = FRT_EXP_SAH_BINS;
    const Box *box;                          // per slot
    std::vector<double> cen;                 // 3 per slot
    std::vector<int32_t> idx;                // slots, partitioned in place
    Nodes out;

    explicit Binned(const std::vector<Box> &b) : box(b.data()), cen(3 * b.size()), idx(b.size()), out(b.size())
    {
        for (size_t i = 0; i < b.size(); ++i) {
            idx[i] = (int32_t)i;
            for (int k = 0; k < 3; ++k) cen[3 * i + k] = 0.5 * (b[i].lo[k] + b[i].hi[k]);
        }
    }
    // node over idx[b, e)
    int32_t build(int b, int e, int depth, int &levels)
    {
        const int me = out.count.fetch_add(1);
        Box nb = box[idx[b]];
        double clo[3], chi[3];
        for (int k = 0; k < 3; ++k) clo[k] = chi[k] = cen[3 * idx[b] + k];
        for (int i = b + 1; i < e; ++i) {
            nb = surround(nb, box[idx[i]]);
            for (int k = 0; k < 3; ++k) {
                clo[k] = std::fmin(clo[k], cen[3 * idx[i] + k]);
                chi[k] = std::fmax(chi[k], cen[3 * idx[i] + k]);
            }
        }
        const int n = e - b;
        int mid = b + n / 2;
        if (n > 2) {
            double best = INFINITY;
            int best_axis = -1, best_bin = 0;
            for (int axis = 0; axis < 3; ++axis) {
                const double ext = chi[axis] - clo[axis];
                if (!(ext > 0)) continue;
                Box bb[kBins];
                int cnt[kBins] = {};
                const double sc = kBins / ext;
                for (int i = b; i < e; ++i) {
                    const int bi = std::min(kBins - 1, (int)((cen[3 * idx[i] + axis] - clo[axis]) * sc));
                    bb[bi] = cnt[bi]++ ? surround(bb[bi], box[idx[i]]) : box[idx[i]];
                }
                double right_area[kBins];
                int right_cnt[kBins];
                Box acc{};
                int c = 0;
                for (int i = kBins - 1; i > 0; --i) {
                    if (cnt[i]) { acc = c ? surround(acc, bb[i]) : bb[i]; c += cnt[i]; }
                    right_area[i] = c ? box_area(acc) : 0.0;
                    right_cnt[i] = c;
                }
                c = 0;
                for (int i = 0; i < kBins - 1; ++i) {
                    if (cnt[i]) { acc = c ? surround(acc, bb[i]) : bb[i]; c += cnt[i]; }
                    if (c == 0 || right_cnt[i + 1] == 0) continue;
                    const double cost = c * box_area(acc) + right_cnt[i + 1] * right_area[i + 1];
                    if (cost < best) { best = cost; best_axis = axis; best_bin = i; }
                }
            }
            if (best_axis >= 0) {
                const double sc = kBins / (chi[best_axis] - clo[best_axis]);
                int32_t *m = std::partition(idx.data() + b, idx.data() + e, [&](int32_t p) {
                    return std::min(kBins - 1, (int)((cen[3 * p + best_axis] - clo[best_axis]) * sc)) <= best_bin;
                });
                mid = (int)(m - idx.data());
            }
            if (mid == b || mid == e) mid = b + n / 2;     // all centroids in one bin: median split
        }
        return out.close(
            me, nb, n, depth, levels, [&](int &lv) { return (mid - b == 1) ? ~idx[b] : build(b, mid, depth + 1, lv); },
            [&](int &lv) { return (e - mid == 1) ? ~idx[mid] : build(mid, e, depth + 1, lv); });
    }
};

}  // namespace

// leaves hold the slot index; the caller maps slots back to prim refs
Tree build_sweep(const std::vector<Box> &boxes)
{
    const int n = (int)boxes.size();
    Sweep s{boxes.data(), Nodes(boxes.size())};
    std::vector<int32_t> slots(n);
    for (int i = 0; i < n; ++i) slots[i] = i;
    Tree t;
    t.root = s.build(slots.data(), n, 1, t.depth);
    t.node_box = std::move(s.out.box);
    t.node_child = std::move(s.out.child);
    return t;
}

Tree build_binned(const std::vector<Box> &boxes)
{
    Binned b(boxes);
    Tree t;
    t.root = b.build(0, (int)boxes.size(), 1, t.depth);
    t.node_box = std::move(b.out.box);
    t.node_child = std::move(b.out.child);
    return t;
}

}  // namespace frt_bvh
