// tree_refine.cpp -- see tree_refine.hpp.  The cost counter restates the visit
// rule of bvh2_step and leaf_hit (csrc/frt_path.hpp) over precomputed slab and
// hit distances; the search moves subtrees and keeps what lowers the count.
#include "tree_refine.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <utility>
#include <vector>

#include "frt.h"

namespace frt_refine {
namespace {

constexpr int kMaxLevels = 64;   // traversal stack of the counter; callers keep trees far shallower
constexpr int kChunks = 16;      // a candidate is scored chunk by chunk and dropped once it falls behind
constexpr double kSlack = 0.002; // ... by this share of the kept tree's whole cost

// Slab tables of every slot of a tree: [ray][slot][6], a ray's records side by
// side.  A candidate differs from the kept tree in the interior nodes on two
// root paths (`dirty`, children before parents); their records are made per
// ray on the way, so a candidate dropped early costs only the rays it saw.
struct Tables {
    int n_slots = 0;
    std::vector<float> tab;
};

inline void unite(const float *a, const float *b, float *out)   // all six entries are minima
{
    for (int k = 0; k < 6; ++k) out[k] = std::min(a[k], b[k]);
}

// rays [r0, r1) on tree t; adds to V and T.  local_of[slot] >= 0: a dirty slot
void count_rays(const Topology &t, const RaySet &R, const Tables &tb, const int *dirty, int n_dirty, const int *local_of,
                int r0, int r1, uint64_t &V, uint64_t &T)
{
    const int L = t.n_leaves;
    const int *child = t.child.data();
    float loc[2 * kMaxLevels][6];
    for (int r = r0; r < r1; ++r) {
        if (!R.live[r]) continue;
        const float *base = &tb.tab[(size_t)r * tb.n_slots * 6];
        auto rec = [&](int s) { return n_dirty > 0 && local_of[s] >= 0 ? loc[local_of[s]] : base + 6 * s; };
        for (int k = 0; k < n_dirty; ++k) {
            const int j = dirty[k] - L;
            unite(rec(child[2 * j]), rec(child[2 * j + 1]), loc[k]);
        }
        const float tmin = R.tmin[r];
        const bool any = R.anyhit[r] != 0;
        const float *pt = &R.prim_t[(size_t)r * R.n_prims];
        float tb_ = R.tmax[r];
        int hp = -1, sp = 0, node = R.root.empty() ? t.root : R.root[r];
        int stk[kMaxLevels];
        for (;;) {
            while (node >= L) {   // interior node: bvh2_step's visit
                ++V;
                const int c0 = child[2 * (node - L)], c1 = child[2 * (node - L) + 1];
                const float *a = rec(c0), *b = rec(c1);
                const float t0 = std::max(std::max(a[0], a[1]), std::max(a[2], tmin));
                const float f0 = std::min(std::min(-a[3], -a[4]), std::min(-a[5], tb_));
                const float t1 = std::max(std::max(b[0], b[1]), std::max(b[2], tmin));
                const float f1 = std::min(std::min(-b[3], -b[4]), std::min(-b[5], tb_));
                const bool h0 = t0 <= f0, h1 = t1 <= f1;
                if (h0 && h1) {
                    const bool first0 = t0 <= t1;
                    stk[sp++] = first0 ? c1 : c0;
                    node = first0 ? c0 : c1;
                } else if (h0) {
                    node = c0;
                } else if (h1) {
                    node = c1;
                } else {
                    node = sp > 0 ? stk[--sp] : -1;
                }
            }
            if (node < 0) break;
            bool done = false;   // leaf_hit: the leaf's primitives in order, t_best and the tie rule
            for (int k = R.prim_first[node]; k < R.prim_first[node + 1]; ++k) {
                ++T;
                const float th = pt[k];
                const int ref = R.prim_ref[k];
                const bool sph = (ref & FRT_PRIM_SPHERE) != 0;
                if (th > 0.0f && th <= tb_ && (th < tb_ || (sph ? hp >= 0 : ref < hp))) {
                    tb_ = th;
                    hp = ref;
                    if (any) { done = true; break; }
                }
            }
            if (done || sp == 0) break;
            node = stk[--sp];
        }
    }
}

void build_tables(const Topology &t, const RaySet &R, Tables &tb)
{
    const int L = t.n_leaves, nI = (int)(t.child.size() / 2);
    tb.n_slots = L + nI;
    tb.tab.resize((size_t)R.n * tb.n_slots * 6);
    // children before parents: a post-order walk from every root a ray starts at (a second root may
    // share subtrees with the first, so a node is taken once)
    std::vector<int> order, roots{t.root};
    roots.insert(roots.end(), R.root.begin(), R.root.end());
    std::sort(roots.begin(), roots.end());
    roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
    std::vector<char> seen(tb.n_slots, 0);
    std::vector<std::pair<int, bool>> st;   // (slot, children done)
    for (int root : roots) st.push_back({root, false});
    while (!st.empty()) {
        const auto [s, done] = st.back();
        st.pop_back();
        if (s < L) continue;
        if (done) { order.push_back(s); continue; }
        if (seen[s]) continue;
        seen[s] = 1;
        st.push_back({s, true});
        st.push_back({t.child[2 * (s - L)], false});
        st.push_back({t.child[2 * (s - L) + 1], false});
    }
    for (int r = 0; r < R.n; ++r) {
        float *base = &tb.tab[(size_t)r * tb.n_slots * 6];
        memcpy(base, &R.slab[(size_t)r * L * 6], sizeof(float) * 6 * L);
        for (size_t k = 0; k < order.size(); ++k) {
            const int s = order[k], j = s - L;
            unite(base + 6 * t.child[2 * j], base + 6 * t.child[2 * j + 1], base + 6 * s);
        }
    }
}

}   // namespace

int Topology::depth() const
{
    int d = 0, sp = 0;
    int st[2 * kMaxLevels][2];
    st[sp][0] = root; st[sp++][1] = 1;
    while (sp > 0) {
        const int s = st[--sp][0], lvl = st[sp][1];
        if (s < n_leaves) continue;
        d = std::max(d, lvl);
        if (lvl >= kMaxLevels) return lvl;   // deeper than any tree the pass handles
        st[sp][0] = child[2 * (s - n_leaves)]; st[sp++][1] = lvl + 1;
        st[sp][0] = child[2 * (s - n_leaves) + 1]; st[sp++][1] = lvl + 1;
    }
    return d;
}

Cost tree_cost(const Topology &t, const RaySet &R)
{
    Tables tb;
    build_tables(t, R, tb);
    uint64_t V = 0, T = 0;
    count_rays(t, R, tb, nullptr, 0, nullptr, 0, R.n, V, T);
    Cost c;
    if (R.n > 0) { c.V = (double)V / R.n; c.T = (double)T / R.n; }
    return c;
}

int refine(Topology &t, const RaySet &R, double w, int max_depth, int max_evals)
{
    const int L = t.n_leaves, nI = L - 1, nS = L + nI;
    if (nI < 2 || R.n <= 0 || max_depth >= kMaxLevels) return 0;
    Tables tb;
    std::vector<int> parent(nS, -1), local_of(nS, -1);
    // chunk bounds and the running cost of the tree kept so far at each bound
    int bound[kChunks + 1];
    for (int c = 0; c <= kChunks; ++c) bound[c] = (int)((int64_t)R.n * c / kChunks);
    double prefix[kChunks + 1] = {0.0};
    auto keep_tree = [&]() {   // parents, tables and prefix costs of t
        std::fill(parent.begin(), parent.end(), -1);
        for (int j = 0; j < nI; ++j) { parent[t.child[2 * j]] = L + j; parent[t.child[2 * j + 1]] = L + j; }
        build_tables(t, R, tb);
        uint64_t V = 0, T = 0;
        for (int c = 0; c < kChunks; ++c) {
            count_rays(t, R, tb, nullptr, 0, nullptr, bound[c], bound[c + 1], V, T);
            prefix[c + 1] = (double)V + w * (double)T;
        }
    };
    keep_tree();
    auto in_subtree = [&](int x, int s) {   // x inside the subtree of s
        for (; x >= 0; x = parent[x]) if (x == s) return true;
        return false;
    };
    auto side_of = [&](int par, int c) { return 2 * (par - L) + (t.child[2 * (par - L)] == c ? 0 : 1); };
    // remove s (its sibling q takes the place of their parent p), then p becomes the
    // parent of (x, s) where x was; returns p's old parent
    auto move = [&](int s, int x) {
        const int p = parent[s];
        const int q = t.child[side_of(p, s) ^ 1];
        const int g = parent[p];
        if (g < 0) t.root = q;
        else t.child[side_of(g, p)] = q;
        parent[q] = g;
        const int xp = parent[x];
        if (xp < 0) t.root = p;
        else t.child[side_of(xp, x)] = p;
        parent[p] = xp;
        t.child[2 * (p - L)] = x;
        t.child[2 * (p - L) + 1] = s;
        parent[x] = p;
        parent[s] = p;
        return g;
    };
    int evals = 0, kept = 0;
    bool improved = true;
    while (improved && evals < max_evals) {
        improved = false;
        for (int s = 0; s < nS && evals < max_evals; ++s) {
            if (parent[s] < 0) continue;   // the root
            int best_x = -1;
            double best_j = prefix[kChunks];
            const Topology keep = t;
            const std::vector<int> keep_parent = parent;
            const int p = parent[s], q = t.child[side_of(p, s) ^ 1];
            for (int x = 0; x < nS && evals < max_evals; ++x) {
                if (x == p || x == q || in_subtree(x, s)) continue;   // q: the same tree again
                const int g = move(s, x);
                if (t.depth() <= max_depth) {
                    ++evals;
                    // the nodes whose leaf sets changed: p, g and their ancestors, deepest first
                    std::pair<int, int> dl[2 * kMaxLevels];   // (-level, slot)
                    int nd = 0;
                    for (int start : {p, g})
                        for (int y = start; y >= 0; y = parent[y]) {
                            int lvl = 0;
                            for (int z = y; z >= 0; z = parent[z]) ++lvl;
                            dl[nd++] = {-lvl, y};
                        }
                    std::sort(dl, dl + nd);
                    nd = (int)(std::unique(dl, dl + nd) - dl);
                    int dirty[2 * kMaxLevels];
                    for (int k = 0; k < nd; ++k) { dirty[k] = dl[k].second; local_of[dirty[k]] = k; }
                    uint64_t V = 0, T = 0;
                    const double slack = kSlack * prefix[kChunks];
                    double j = 0.0;
                    bool ok = true;
                    for (int c = 0; c < kChunks && ok; ++c) {
                        count_rays(t, R, tb, dirty, nd, local_of.data(), bound[c], bound[c + 1], V, T);
                        j = (double)V + w * (double)T;
                        ok = j <= prefix[c + 1] + slack;
                    }
                    for (int k = 0; k < nd; ++k) local_of[dirty[k]] = -1;
                    if (ok && j < best_j) { best_j = j; best_x = x; }
                }
                t = keep;
                parent = keep_parent;
            }
            if (best_x < 0) continue;
            move(s, best_x);   // the best place found for s
            keep_tree();
            ++kept;
            improved = true;
        }
    }
    return kept;
}

}   // namespace frt_refine
