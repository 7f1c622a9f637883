// Binned-SAH BVH2 builder (host) — see pg_bvh.h.  buildBinary's greedy top-down tree is reoptimised by subtree
// reinsertion (Reinserter; PG_BVH_REINSERT=0: not) before the 8-wide and 4-wide trees are collapsed from it: on C3
// the binary tree's SAH cost falls 16.95 -> 14.47, the closest-hit walk visits 17 % fewer nodes per ray and k_rays
// takes 7.5 % less time (profiles/r21_bvh_reinsert).
#include "pg_bvh.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "pg_layout.h"

namespace pgh {
namespace {

struct Box {
    float lo[3] = {std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity(),
                   std::numeric_limits<float>::infinity()};
    float hi[3] = {-std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                   -std::numeric_limits<float>::infinity()};
    void grow(const float *p) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], p[a]);
            hi[a] = std::max(hi[a], p[a]);
        }
    }
    void grow(const Box &b) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], b.lo[a]);
            hi[a] = std::max(hi[a], b.hi[a]);
        }
    }
    float area() const {
        float e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
        if (!(e0 >= 0)) return 0.0f;
        return 2.0f * (e0 * e1 + e1 * e2 + e2 * e0);
    }
};

struct BNode {
    Box box;
    int32_t child[2] = {-1, -1};  // build-node indices (inner)
    uint32_t first = 0, count = 0;
    bool leaf = false;
};

constexpr int kBins = 32;
// SAH constants: leaves of at most kLeafTarget triangles are never split; a triangle test costs
// kTriCost node traversals.  PG_BVH_LEAF_TARGET / PG_BVH_TRI_COST override them (A/B measurements).
uint32_t leafTarget() {
    const char *e = std::getenv("PG_BVH_LEAF_TARGET");
    return e ? (uint32_t)std::atoi(e) : 2u;
}
float triCost() {
    const char *e = std::getenv("PG_BVH_TRI_COST");
    return e ? (float)std::atof(e) : 1.0f;
}

}  // namespace

// Binned-SAH binary build: nodes bn (bn[0] = root), triangle permutation ord, leaves of at most
// maxLeaf triangles (SAH leaf/split decision, object median past depth 32).
static void buildBinary(const float *P, const uint32_t *I, uint32_t nt, uint32_t maxLeaf, std::vector<BNode> &bn,
                 std::vector<uint32_t> &ord, uint32_t &maxDepth, Box &all) {
    std::vector<Box> tb(nt);
    std::vector<float> cen(3 * (size_t)nt);
    all = Box();
    for (uint32_t t = 0; t < nt; ++t) {
        for (int j = 0; j < 3; ++j) tb[t].grow(P + 3 * (size_t)I[3 * (size_t)t + j]);
        for (int a = 0; a < 3; ++a) cen[3 * (size_t)t + a] = 0.5f * (tb[t].lo[a] + tb[t].hi[a]);
        all.grow(tb[t]);
    }
    ord.assign(nt, 0);
    for (uint32_t t = 0; t < nt; ++t) ord[t] = t;
    bn.clear();
    const uint32_t kLeafTarget = std::max(1u, leafTarget());
    const float kTri = triCost();
    bn.reserve(nt ? 2 * (size_t)nt / kLeafTarget + 8 : 8);
    struct Job { int32_t node; uint32_t first, count, depth; };
    std::vector<Job> st;
    bn.emplace_back();
    st.push_back({0, 0, nt, 0});
    maxDepth = 0;
    while (!st.empty()) {
        Job j = st.back();
        st.pop_back();
        maxDepth = std::max(maxDepth, j.depth);
        Box box, cb;
        for (uint32_t i = j.first; i < j.first + j.count; ++i) {
            box.grow(tb[ord[i]]);
            cb.grow(&cen[3 * (size_t)ord[i]]);
        }
        bn[j.node].box = box;
        uint32_t mid = 0;
        bool leaf = j.count <= std::min(kLeafTarget, maxLeaf);
        if (!leaf) {
            int bestAxis = -1, bestBin = -1;
            float bestCost = std::numeric_limits<float>::infinity();
            const bool median = j.depth >= 32;  // bound the depth: object-median splits from here on
            if (!median) {
                for (int ax = 0; ax < 3; ++ax) {
                    float lo = cb.lo[ax], hi = cb.hi[ax];
                    if (!(hi > lo)) continue;
                    float k = kBins / (hi - lo);
                    Box bb[kBins];
                    uint32_t bc[kBins] = {0};
                    for (uint32_t i = j.first; i < j.first + j.count; ++i) {
                        int b = std::min(kBins - 1, std::max(0, (int)((cen[3 * (size_t)ord[i] + ax] - lo) * k)));
                        bb[b].grow(tb[ord[i]]);
                        bc[b]++;
                    }
                    float la[kBins];
                    uint32_t lc[kBins];
                    Box acc;
                    uint32_t n = 0;
                    for (int b = 0; b < kBins; ++b) {
                        acc.grow(bb[b]);
                        n += bc[b];
                        la[b] = acc.area();
                        lc[b] = n;
                    }
                    acc = Box();
                    n = 0;
                    for (int b = kBins - 1; b > 0; --b) {
                        acc.grow(bb[b]);
                        n += bc[b];
                        if (lc[b - 1] == 0 || n == 0) continue;
                        float cost = la[b - 1] * lc[b - 1] + acc.area() * n;
                        if (cost < bestCost) {
                            bestCost = cost;
                            bestAxis = ax;
                            bestBin = b;
                        }
                    }
                }
                float leafCost = box.area() * (float)j.count * kTri;
                float splitCost = box.area() * 1.0f + bestCost * kTri;  // one node visit + the children's tests
                if (bestAxis >= 0 && splitCost >= leafCost && j.count <= maxLeaf) leaf = true;
            }
            if (!leaf) {
                if (bestAxis >= 0 && !median) {
                    float lo = cb.lo[bestAxis], hi = cb.hi[bestAxis];
                    float k = kBins / (hi - lo);
                    auto it = std::partition(ord.begin() + j.first, ord.begin() + j.first + j.count, [&](uint32_t t) {
                        int b = std::min(kBins - 1, std::max(0, (int)((cen[3 * (size_t)t + bestAxis] - lo) * k)));
                        return b < bestBin;
                    });
                    mid = (uint32_t)(it - ord.begin());
                }
                if (bestAxis < 0 || median || mid == j.first || mid == j.first + j.count) {
                    if (j.count <= maxLeaf && bestAxis < 0 && !median) {
                        leaf = true;  // coincident centroids, small enough
                    } else {
                        int ax = 0;
                        float ext = -1;
                        for (int a = 0; a < 3; ++a)
                            if (cb.hi[a] - cb.lo[a] > ext) {
                                ext = cb.hi[a] - cb.lo[a];
                                ax = a;
                            }
                        mid = j.first + j.count / 2;
                        std::nth_element(ord.begin() + j.first, ord.begin() + mid, ord.begin() + j.first + j.count,
                                         [&](uint32_t a, uint32_t b) {
                                             return cen[3 * (size_t)a + ax] < cen[3 * (size_t)b + ax];
                                         });
                    }
                }
            }
        }
        if (leaf) {
            bn[j.node].leaf = true;
            bn[j.node].first = j.first;
            bn[j.node].count = j.count;
        } else {
            int32_t l = (int32_t)bn.size();
            bn.emplace_back();
            bn.emplace_back();
            bn[j.node].child[0] = l;
            bn[j.node].child[1] = l + 1;
            st.push_back({l + 1, mid, j.first + j.count - mid, j.depth + 1});
            st.push_back({l, j.first, mid - j.first, j.depth + 1});
        }
    }
}

namespace {

// 0: the tree of buildBinary as it is; 1 (default): reoptimised by reinsertion; 2: reoptimise, then behave as
// if a collapse had refused the result (the fallback of buildBvh, for its test)
int reinsertMode() {
    const char *e = std::getenv("PG_BVH_REINSERT");
    return e ? std::atoi(e) : 1;
}

// At most this many sweeps over all inner nodes.  A sweep ends at its first batch (1 % of the nodes, in priority
// order) that gains 0.1 % of the cost or less, so a sweep costs a few batches: the 1.0 M-triangle kitchen builds
// in 1.3 x the time of the plain build, and no smaller limit by node count is needed.
constexpr uint32_t kReinsertSweeps = 3;

// SAH cost of a binary tree relative to its root's area: one visit per inner node, triCost() per leaf triangle
// (the terms of buildBinary's leaf / split decision)
float sahCost(const std::vector<BNode> &bn) {
    const float kTri = triCost();
    double inner = 0.0, leaves = 0.0;
    std::vector<int32_t> s{0};
    while (!s.empty()) {
        const int32_t n = s.back();
        s.pop_back();
        if (bn[n].leaf) {
            leaves += (double)bn[n].box.area() * bn[n].count;
            continue;
        }
        inner += bn[n].box.area();
        s.push_back(bn[n].child[0]);
        s.push_back(bn[n].child[1]);
    }
    const double root = bn[0].box.area();
    return root > 0.0 ? (float)((inner + kTri * leaves) / root) : 0.0f;
}

// Insertion-based reoptimisation of the binary tree (Bittner, Hapala, Havran 2013).  A move takes an inner
// node N out together with its parent (N's sibling takes the parent's place) and puts N's two children back,
// the larger first, each where a branch-and-bound search from the root finds the smallest rise of the summed
// inner-node area; the two freed nodes become the new parents.  Leaves are never opened, so the leaf terms of
// the cost are constant and the cost of a move is the change of `inner`.  A move that does not lower it, or
// that would put a leaf deeper than depthLimit, is undone from the journal.  The root stays node 0 (no node is
// inserted beside it, none of its children is taken out).  No timers, threads or random numbers: candidates
// go in decreasing priority, ties in priority and in insertion cost to the lower node index.
struct Reinserter {
    std::vector<BNode> &bn;
    std::vector<int32_t> parent;
    std::vector<uint32_t> height;  // levels below the node (leaf: 0)
    uint32_t depthLimit;
    double inner = 0.0;   // summed area of the inner nodes
    double leaves = 0.0;  // triCost() * summed area * count of the leaves: constant
    struct Saved { int32_t n; BNode node; int32_t parent; uint32_t height; };
    std::vector<Saved> journal;
    struct Cand { double cost; int32_t n; uint32_t depth; };
    std::vector<Cand> heap;

    Reinserter(std::vector<BNode> &b, uint32_t limit) : bn(b), parent(b.size(), -1), height(b.size(), 0), depthLimit(limit) {
        std::vector<int32_t> pre, s{0};
        while (!s.empty()) {
            const int32_t n = s.back();
            s.pop_back();
            pre.push_back(n);
            if (bn[n].leaf) continue;
            for (int k = 0; k < 2; ++k) {
                parent[bn[n].child[k]] = n;
                s.push_back(bn[n].child[k]);
            }
        }
        for (size_t i = pre.size(); i-- > 0;) {
            const int32_t n = pre[i];
            if (bn[n].leaf) {
                leaves += (double)triCost() * bn[n].box.area() * bn[n].count;
                continue;
            }
            height[n] = 1 + std::max(height[bn[n].child[0]], height[bn[n].child[1]]);
            inner += bn[n].box.area();
        }
    }
    void touch(int32_t n) { journal.push_back({n, bn[n], parent[n], height[n]}); }
    void undo(double innerBefore) {
        for (size_t i = journal.size(); i-- > 0;) {
            const Saved &u = journal[i];
            bn[u.n] = u.node;
            parent[u.n] = u.parent;
            height[u.n] = u.height;
        }
        journal.clear();
        inner = innerBefore;
    }
    // boxes and heights from inner node n up, as far as they change
    void refit(int32_t n) {
        for (; n >= 0; n = parent[n]) {
            const BNode &a = bn[bn[n].child[0]], &b = bn[bn[n].child[1]];
            Box box = a.box;
            box.grow(b.box);
            const uint32_t h = 1 + std::max(height[bn[n].child[0]], height[bn[n].child[1]]);
            if (h == height[n] && std::memcmp(&box, &bn[n].box, sizeof(Box)) == 0) return;
            touch(n);
            inner += (double)box.area() - (double)bn[n].box.area();
            bn[n].box = box;
            height[n] = h;
        }
    }
    static bool before(const Cand &x, const Cand &y) { return x.cost > y.cost || (x.cost == y.cost && x.n > y.n); }
    // the node beside which subtree m costs least: induced cost (area growth of the ancestors) + the area of the
    // new common parent; -1 if the depth limit leaves no place
    int32_t findPlace(int32_t m) {
        const Box &mb = bn[m].box;
        const double mArea = mb.area();
        double best = std::numeric_limits<double>::infinity();
        int32_t bestN = -1;
        heap.clear();
        heap.push_back({0.0, 0, 0});
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end(), before);
            const Cand c = heap.back();
            heap.pop_back();
            if (c.cost + mArea > best) break;  // every later entry induces at least as much
            Box u = bn[c.n].box;
            u.grow(mb);
            const double total = c.cost + (double)u.area();
            if (c.n != 0 && c.depth + 1 + std::max(height[c.n], height[m]) <= depthLimit &&
                (total < best || (total == best && c.n < bestN))) {
                best = total;
                bestN = c.n;
            }
            const double below = total - (double)bn[c.n].box.area();
            if (bn[c.n].leaf || below + mArea > best) continue;
            for (int k = 0; k < 2; ++k) {
                heap.push_back({below, bn[c.n].child[k], c.depth + 1});
                std::push_heap(heap.begin(), heap.end(), before);
            }
        }
        return bestN;
    }
    bool insert(int32_t m, int32_t freeNode) {
        const int32_t x = findPlace(m);
        if (x < 0) return false;
        const int32_t px = parent[x];
        touch(px);
        touch(x);
        touch(freeNode);
        touch(m);
        BNode &f = bn[freeNode];
        f.leaf = false;
        f.first = f.count = 0;
        f.child[0] = x;
        f.child[1] = m;
        f.box = bn[x].box;
        f.box.grow(bn[m].box);
        height[freeNode] = 1 + std::max(height[x], height[m]);
        inner += f.box.area();
        bn[px].child[bn[px].child[0] == x ? 0 : 1] = freeNode;
        parent[freeNode] = px;
        parent[x] = parent[m] = freeNode;
        refit(px);
        return true;
    }
    bool movable(int32_t n) const { return !bn[n].leaf && parent[n] > 0; }
    // true: the move lowered the cost and stays
    bool tryMove(int32_t n) {
        const double innerBefore = inner;
        const int32_t p = parent[n], g = parent[p];
        const int32_t sib = bn[p].child[bn[p].child[0] == n ? 1 : 0];
        int32_t a = bn[n].child[0], b = bn[n].child[1];
        if (bn[b].box.area() > bn[a].box.area()) std::swap(a, b);
        for (int32_t t : {g, p, n, sib, a, b}) touch(t);
        bn[g].child[bn[g].child[0] == p ? 0 : 1] = sib;
        parent[sib] = g;
        parent[n] = parent[p] = parent[a] = parent[b] = -1;
        inner -= (double)bn[n].box.area() + (double)bn[p].box.area();
        refit(g);
        if (insert(a, n) && insert(b, p) && inner < innerBefore) {
            journal.clear();
            return true;
        }
        undo(innerBefore);
        return false;
    }
    // Bittner's combined priority: large nodes whose children fill them badly
    float priority(int32_t n) const {
        const float A = bn[n].box.area(), a = bn[bn[n].child[0]].box.area(), b = bn[bn[n].child[1]].box.area();
        const float tiny = 1e-12f * A;
        return A * (A / std::max(0.5f * (a + b), tiny)) * (A / std::max(std::min(a, b), tiny));
    }
    void run(uint32_t sweeps) {
        std::vector<std::pair<float, int32_t>> cand;
        for (uint32_t s = 0; s < sweeps; ++s) {
            cand.clear();
            for (int32_t n = 0; n < (int32_t)bn.size(); ++n)
                if (movable(n) && bn[n].box.area() > 0.0f) cand.push_back({priority(n), n});
            if (cand.empty()) return;
            std::sort(cand.begin(), cand.end(), [](const std::pair<float, int32_t> &x, const std::pair<float, int32_t> &y) {
                return x.first > y.first || (x.first == y.first && x.second < y.second);
            });
            const size_t batch = std::max<size_t>(1, cand.size() / 100);  // 1 % of the inner nodes
            const double sweepStart = inner;
            for (size_t i = 0; i < cand.size(); i += batch) {
                const double batchStart = inner;
                for (size_t k = i; k < std::min(cand.size(), i + batch); ++k)
                    if (movable(cand[k].second)) tryMove(cand[k].second);  // an earlier move may have made it a root's child
                if (!(batchStart - inner > 1e-3 * (batchStart + leaves))) break;  // this batch gained 0.1 % or less
            }
            if (!(sweepStart - inner > 1e-3 * (sweepStart + leaves))) return;
        }
    }
};

// the triangle order and the leaves' ranges in depth-first order of the tree, child 0 first; the deepest leaf
void emitDepthFirst(std::vector<BNode> &bn, std::vector<uint32_t> &ord, uint32_t &maxDepth) {
    std::vector<uint32_t> out;
    out.reserve(ord.size());
    std::vector<std::pair<int32_t, uint32_t>> s{{0, 0}};
    maxDepth = 0;
    while (!s.empty()) {
        const auto [n, d] = s.back();
        s.pop_back();
        if (!bn[n].leaf) {
            s.push_back({bn[n].child[1], d + 1});
            s.push_back({bn[n].child[0], d + 1});
            continue;
        }
        maxDepth = std::max(maxDepth, d);
        const uint32_t first = (uint32_t)out.size();
        out.insert(out.end(), ord.begin() + bn[n].first, ord.begin() + bn[n].first + bn[n].count);
        bn[n].first = first;
    }
    ord.swap(out);
}

}  // namespace

// TriAccel record of triangle t (TriAccel::load, triaccel.h:37-94, in fp32 as the reference computes
// it; this file builds with -ffp-contract=off): 12 floats, pg_layout.h "Triangle records"
static void triAccelRecord(const float *P, const uint32_t *I, uint32_t t, float *w) {
    static const int waldModulo[4] = {1, 2, 0, 1};
    const float *A = P + 3 * (size_t)I[3 * (size_t)t], *B = P + 3 * (size_t)I[3 * (size_t)t + 1],
                *C = P + 3 * (size_t)I[3 * (size_t)t + 2];
    const float b[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]}, c[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const float N[3] = {c[1] * b[2] - c[2] * b[1], c[2] * b[0] - c[0] * b[2], c[0] * b[1] - c[1] * b[0]};  // cross(c, b)
    int k = 0;
    for (int j = 0; j < 3; ++j)
        if (std::fabs(N[j]) > std::fabs(N[k])) k = j;
    const int u = waldModulo[k], v = waldModulo[k + 1];
    const float n_k = N[k], denom = b[u] * c[v] - b[v] * c[u];
    for (int i = 0; i < 12; ++i) w[i] = 0.0f;
    uint32_t kk = (uint32_t)k;
    if (denom == 0) {  // degenerate: k = 3, a NaN plane that no t passes
        w[0] = w[1] = w[2] = std::numeric_limits<float>::quiet_NaN();
        kk = 3;
    } else {
        w[0] = N[u] / n_k;                                          // n_u
        w[1] = N[v] / n_k;                                          // n_v
        w[2] = (A[0] * N[0] + A[1] * N[1] + A[2] * N[2]) / n_k;    // n_d = dot(A, N) / n_k
        w[4] = A[u];                                                // a_u
        w[5] = A[v];                                                // a_v
        w[6] = b[u] / denom;                                        // b_nu
        w[7] = -b[v] / denom;                                       // b_nv
        w[8] = c[v] / denom;                                        // c_nu
        w[9] = -c[u] / denom;                                       // c_nv
    }
    std::memcpy(&w[3], &kk, 4);
    std::memcpy(&w[10], &t, 4);  // the original triangle id
}

namespace {

// Child-slot assignment by ray octant: slot s holds the child a ray of octant s (bit a set =
// negative direction along axis a) should visit first, i.e. the child minimising
// dot(centroid - parent centroid, diag(s)).  Greedy over the sorted (cost, child, slot) table.
void assignSlots(const Box &parent, const std::vector<Box> &cb, int slotOf[8]) {
    const int k = (int)cb.size();
    float pc[3];
    for (int a = 0; a < 3; ++a) pc[a] = 0.5f * (parent.lo[a] + parent.hi[a]);
    struct C { float cost; int child, slot; };
    std::vector<C> tab;
    for (int i = 0; i < k; ++i) {
        float v[3];
        for (int a = 0; a < 3; ++a) v[a] = 0.5f * (cb[i].lo[a] + cb[i].hi[a]) - pc[a];
        for (int sl = 0; sl < 8; ++sl) {
            float c = 0;
            for (int a = 0; a < 3; ++a) c += ((sl >> a) & 1) ? -v[a] : v[a];
            tab.push_back({c, i, sl});
        }
    }
    std::stable_sort(tab.begin(), tab.end(), [](const C &x, const C &y) { return x.cost < y.cost; });
    bool usedSlot[8] = {false};
    for (int i = 0; i < k; ++i) slotOf[i] = -1;
    for (const C &c : tab) {
        if (slotOf[c.child] >= 0 || usedSlot[c.slot]) continue;
        slotOf[c.child] = c.slot;
        usedSlot[c.slot] = true;
    }
}

// power-of-two scale exponent with 255 * 2^e >= extent
int quantExponent(float extent) {
    if (!(extent > 0)) return -126;
    int e;
    std::frexp((double)extent / 255.0, &e);  // extent/255 = m * 2^e, m in [0.5, 1)
    return std::max(-126, std::min(127, e));
}

}  // namespace

// 8-wide BVH (for any-hit queries), collapsed from the binary tree (bn, ord); its leaf slots copy the
// binary leaves' triangle ranges contiguously, and that copy order (out.order) is the one triangle
// order of both BVHs: posOf[i] = the position of ord[i] in it.
static bool buildWide(const float *P, const uint32_t *I, uint32_t nt, uint32_t stack_limit, const std::vector<BNode> &bn,
                      const std::vector<uint32_t> &ord, BvhOut &out, std::vector<uint32_t> &posOf) {
    // ---- collapse to 8-wide nodes, SAH-optimal over the binary tree (dynamic programming after
    // Ylitie et al. 2017): dist[n][j] = cheapest way to spread subtree n over at most j slots of
    // one wide node; a slot is a leaf (subtree of <= PG_WIDE_LEAF_MAX triangles, one contiguous
    // range of `ord`) or an inner wide node.
    const size_t nb = bn.size();
    constexpr float kCostNode = 1.0f, kCostTri = 0.3f;
    constexpr float kInf = std::numeric_limits<float>::infinity();
    std::vector<uint32_t> rFirst(nb), rCount(nb);
    std::vector<std::array<float, 9>> dist(nb);
    std::vector<float> cWide(nb, kInf), cLeaf(nb, kInf);
    std::vector<std::array<uint8_t, 9>> splitK(nb);  // best left share for dist[n][j], 0 = n as one slot
    {
        std::vector<int32_t> post;
        std::vector<int32_t> s{0};
        while (!s.empty()) {
            int32_t n = s.back();
            s.pop_back();
            post.push_back(n);
            if (!bn[n].leaf) {
                s.push_back(bn[n].child[0]);
                s.push_back(bn[n].child[1]);
            }
        }
        for (size_t i = post.size(); i-- > 0;) {
            const int32_t n = post[i];
            const float A = bn[n].box.area();
            splitK[n].fill(0);
            if (bn[n].leaf) {
                rFirst[n] = bn[n].first;
                rCount[n] = bn[n].count;
                cLeaf[n] = kCostTri * A * (float)bn[n].count;
                for (int j = 1; j <= 8; ++j) dist[n][j] = cLeaf[n];
                continue;
            }
            const int32_t L = bn[n].child[0], R = bn[n].child[1];
            rFirst[n] = std::min(rFirst[L], rFirst[R]);
            rCount[n] = rCount[L] + rCount[R];
            if (rCount[n] <= PG_WIDE_LEAF_MAX) cLeaf[n] = kCostTri * A * (float)rCount[n];
            // n opened as a wide node: its children spread over 8 slots
            float best = kInf;
            for (int k = 1; k < 8; ++k) best = std::min(best, dist[L][k] + dist[R][8 - k]);
            cWide[n] = kCostNode * A + best;
            dist[n][1] = std::min(cLeaf[n], cWide[n]);
            for (int j = 2; j <= 8; ++j) {
                dist[n][j] = dist[n][1];
                for (int k = 1; k < j; ++k) {
                    const float c = dist[L][k] + dist[R][j - k];
                    if (c < dist[n][j]) {
                        dist[n][j] = c;
                        splitK[n][j] = (uint8_t)k;
                    }
                }
            }
        }
    }
    // slots of wide node n: children of n spread over 8 slots along the DP's choices
    auto collect = [&](int32_t n, std::vector<int32_t> &out) {
        std::vector<std::pair<int32_t, int>> s;
        int bestK = 1;
        float best = kInf;
        for (int k = 1; k < 8; ++k) {
            const float c = dist[bn[n].child[0]][k] + dist[bn[n].child[1]][8 - k];
            if (c < best) {
                best = c;
                bestK = k;
            }
        }
        s.push_back({bn[n].child[1], 8 - bestK});
        s.push_back({bn[n].child[0], bestK});
        while (!s.empty()) {
            auto [m, j] = s.back();
            s.pop_back();
            const int k = bn[m].leaf ? 0 : splitK[m][j];
            if (k == 0) {
                out.push_back(m);
            } else {
                s.push_back({bn[m].child[1], j - k});
                s.push_back({bn[m].child[0], k});
            }
        }
    };
    // a slot is a leaf when the subtree fits one and a leaf is not costlier than a wide node
    auto isLeafSlot = [&](int32_t m) { return bn[m].leaf || cLeaf[m] <= cWide[m]; };

    struct WTask { int32_t bnode; uint32_t wide; uint32_t depth; };
    std::vector<WTask> work{{0, 0, 1}};
    std::vector<float> nodes(PG_WIDE_NODE_F4 * 4, 0.0f);
    std::vector<uint32_t> order;
    posOf.assign(nt, 0);
    order.reserve(nt);
    uint32_t wideDepth = 0;
    for (size_t w = 0; w < work.size(); ++w) {
        const WTask task = work[w];
        wideDepth = std::max(wideDepth, task.depth);
        std::vector<int32_t> ch;
        if (isLeafSlot(task.bnode)) ch.push_back(task.bnode);  // tiny scene: the root is one leaf
        else collect(task.bnode, ch);
        std::vector<Box> cb;
        Box parent;
        for (int32_t c : ch) {
            cb.push_back(bn[c].box);
            parent.grow(bn[c].box);
        }
        int slotOf[8];
        assignSlots(parent, cb, slotOf);
        int childAt[8];
        for (int sl = 0; sl < 8; ++sl) childAt[sl] = -1;
        for (size_t i = 0; i < ch.size(); ++i) childAt[slotOf[i]] = (int)i;
        // quantisation frame of this node
        int ex[3];
        float scale[3];
        for (int a = 0; a < 3; ++a) {
            ex[a] = quantExponent(parent.hi[a] - parent.lo[a]);
            scale[a] = std::ldexp(1.0f, ex[a]);
        }
        uint32_t imask = 0, childBase = (uint32_t)(nodes.size() / (PG_WIDE_NODE_F4 * 4)),
                 triBase = (uint32_t)order.size(), nInner = 0;
        uint8_t meta[8] = {0}, q[6][8];
        for (int a = 0; a < 6; ++a)
            for (int sl = 0; sl < 8; ++sl) q[a][sl] = 0;
        for (int sl = 0; sl < 8; ++sl) {
            const int i = childAt[sl];
            if (i < 0) continue;
            const int32_t cn = ch[i];
            const BNode &c = bn[cn];
            for (int a = 0; a < 3; ++a) {
                // conservative: floor / ceil in double, then checked against the float reconstruction
                double lo = std::floor(((double)c.box.lo[a] - parent.lo[a]) / scale[a]);
                double hi = std::ceil(((double)c.box.hi[a] - parent.lo[a]) / scale[a]);
                lo = std::max(0.0, std::min(255.0, lo));
                hi = std::max(0.0, std::min(255.0, hi));
                while (lo > 0 && parent.lo[a] + (float)lo * scale[a] > c.box.lo[a]) lo -= 1;
                while (hi < 255 && parent.lo[a] + (float)hi * scale[a] < c.box.hi[a]) hi += 1;
                q[a][sl] = (uint8_t)lo;
                q[3 + a][sl] = (uint8_t)hi;
            }
            if (isLeafSlot(cn)) {
                const uint32_t off = (uint32_t)order.size() - triBase;
                for (uint32_t k = 0; k < rCount[cn]; ++k) {
                    posOf[rFirst[cn] + k] = (uint32_t)order.size();
                    order.push_back(ord[rFirst[cn] + k]);
                }
                meta[sl] = (uint8_t)(off | (rCount[cn] << 5));  // count 1..3 in bits 5-6 (0 = empty slot)
            } else {
                imask |= 1u << sl;
                work.push_back({cn, childBase + nInner, task.depth + 1});
                ++nInner;
            }
        }
        nodes.resize(nodes.size() + (size_t)nInner * PG_WIDE_NODE_F4 * 4, 0.0f);
        float *o = &nodes[(size_t)task.wide * PG_WIDE_NODE_F4 * 4];
        uint32_t w0 = (uint32_t)(ex[0] + 127) | ((uint32_t)(ex[1] + 127) << 8) | ((uint32_t)(ex[2] + 127) << 16) |
                      (imask << 24);
        o[0] = parent.lo[0];
        o[1] = parent.lo[1];
        o[2] = parent.lo[2];
        std::memcpy(&o[3], &w0, 4);
        uint32_t w1[4] = {childBase, triBase, 0, 0};
        std::memcpy(&w1[2], meta, 8);
        std::memcpy(&o[4], w1, 16);
        // [2] qlo.x qlo.y  [3] qlo.z qhi.x  [4] qhi.y qhi.z   (8 bytes each, slot order)
        std::memcpy(&o[8], q[0], 8);
        std::memcpy(&o[10], q[1], 8);
        std::memcpy(&o[12], q[2], 8);
        std::memcpy(&o[14], q[3], 8);
        std::memcpy(&o[16], q[4], 8);
        std::memcpy(&o[18], q[5], 8);
    }
    out.wnodes.swap(nodes);
    out.wide_depth = wideDepth;
    if (wideDepth + 1 > stack_limit || order.size() != nt) return false;
    out.order.swap(order);
    out.tris.assign(4 * (size_t)PG_TRI_F4(nt), 0.0f);
    for (uint32_t k = 0; k < nt; ++k) {
        float rec[12];
        triAccelRecord(P, I, out.order[k], rec);
        for (uint32_t r = 0; r < 3; ++r) std::memcpy(&out.tris[4 * (size_t)PG_TRI_ROW(k, r)], rec + 4 * r, 16);
    }
    return true;
}

// one 4-wide node (pg_layout.h PG_QNODE_*): child boxes box[2a][s] / box[2a+1][s] (lo / hi along axis
// a) of the first `used` slots, refs r[4]; the planes as bytes in the
// node's frame rounded outward as the 8-wide nodes' are
static void putQuadNode(float *o, const float box[6][4], const int32_t r[4], int used) {
    Box parent;
    if (used == 0)
        for (int a = 0; a < 3; ++a) parent.lo[a] = parent.hi[a] = 0.0f;
    for (int s = 0; s < used; ++s)
        for (int a = 0; a < 3; ++a) {
            parent.lo[a] = std::min(parent.lo[a], box[2 * a][s]);
            parent.hi[a] = std::max(parent.hi[a], box[2 * a + 1][s]);
        }
    uint32_t e = 0, w[6] = {0, 0, 0, 0, 0, 0};
    for (int a = 0; a < 3; ++a) {
        const int ex = quantExponent(parent.hi[a] - parent.lo[a]);
        const float scale = std::ldexp(1.0f, ex);
        e |= (uint32_t)(ex + 127) << (8 * a);
        o[a] = parent.lo[a];
        for (int s = 0; s < 4; ++s) {
            double lo = 255, hi = 0;  // empty slot: an inverted box
            if (s < used) {
                lo = std::floor(((double)box[2 * a][s] - parent.lo[a]) / scale);
                hi = std::ceil(((double)box[2 * a + 1][s] - parent.lo[a]) / scale);
                lo = std::max(0.0, std::min(255.0, lo));
                hi = std::max(0.0, std::min(255.0, hi));
                while (lo > 0 && parent.lo[a] + (float)lo * scale > box[2 * a][s]) lo -= 1;
                while (hi < 255 && parent.lo[a] + (float)hi * scale < box[2 * a + 1][s]) hi += 1;
            }
            w[2 * a] |= (uint32_t)lo << (8 * s);
            w[2 * a + 1] |= (uint32_t)hi << (8 * s);
        }
    }
    std::memcpy(&o[3], &e, 4);
    std::memcpy(&o[4], r, 16);
    std::memcpy(&o[8], w, 24);
    o[14] = o[15] = 0.0f;
}

// 4-wide BVH (closest hit) over the same tree; its leaves are the binary leaves (same refs).
// Which binary nodes a 4-wide node absorbs is the SAH-optimal choice (the 8-wide collapse's dynamic
// programme with 4 slots and the leaves fixed: it minimises the summed surface area of the opened
// nodes, i.e. the expected node visits); PG_BVH4_GREEDY=1 opens the largest-area inner child
// instead (A/B).  Siblings are stored consecutively, nodes depth first.  Fails if a root-to-leaf walk
// could hold more than PG_QSTACK_DEPTH stack entries (the siblings pushed at every level).
static bool buildQuadBvh(const std::vector<BNode> &bn, const std::vector<uint32_t> &posOf, BvhOut &out) {
    const bool greedy = std::getenv("PG_BVH4_GREEDY") && std::atoi(std::getenv("PG_BVH4_GREEDY")) != 0;
    const size_t nb = bn.size();
    constexpr float kInf = std::numeric_limits<float>::infinity();
    // dist[n][j]: least summed area of opened nodes to spread subtree n over at most j slots
    std::vector<std::array<float, 5>> dist(nb);
    std::vector<std::array<uint8_t, 5>> splitK(nb);
    {
        std::vector<int32_t> post, s{0};
        while (!s.empty()) {
            const int32_t n = s.back();
            s.pop_back();
            post.push_back(n);
            if (!bn[n].leaf) {
                s.push_back(bn[n].child[0]);
                s.push_back(bn[n].child[1]);
            }
        }
        for (size_t i = post.size(); i-- > 0;) {
            const int32_t n = post[i];
            splitK[n].fill(0);
            if (bn[n].leaf) {
                dist[n].fill(0.0f);
                continue;
            }
            const int32_t L = bn[n].child[0], R = bn[n].child[1];
            float best = kInf;
            for (int k = 1; k < 4; ++k) best = std::min(best, dist[L][k] + dist[R][4 - k]);
            dist[n][1] = bn[n].box.area() + best;  // n as one slot: an opened 4-wide node
            for (int j = 2; j <= 4; ++j) {
                dist[n][j] = dist[n][1];
                for (int k = 1; k < j; ++k) {
                    const float c = dist[L][k] + dist[R][j - k];
                    if (c < dist[n][j]) {
                        dist[n][j] = c;
                        splitK[n][j] = (uint8_t)k;
                    }
                }
            }
        }
    }
    // the slots of opened node n along the programme's choices
    auto collect = [&](int32_t n, std::vector<int32_t> &ch) {
        int bestK = 1;
        float best = kInf;
        for (int k = 1; k < 4; ++k) {
            const float c = dist[bn[n].child[0]][k] + dist[bn[n].child[1]][4 - k];
            if (c < best) {
                best = c;
                bestK = k;
            }
        }
        std::vector<std::pair<int32_t, int>> s{{bn[n].child[1], 4 - bestK}, {bn[n].child[0], bestK}};
        while (!s.empty()) {
            auto [m, j] = s.back();
            s.pop_back();
            const int k = bn[m].leaf ? 0 : splitK[m][j];
            if (k == 0) {
                ch.push_back(m);
            } else {
                s.push_back({bn[m].child[1], j - k});
                s.push_back({bn[m].child[0], k});
            }
        }
    };
    auto ref = [&](int32_t n, int32_t inner) -> int32_t {
        if (bn[n].leaf) return (int32_t)(~((posOf[bn[n].first] << 4) | bn[n].count));
        return inner;
    };
    struct QTask { int32_t bnode; uint32_t qnode; uint32_t stackNeed; };
    std::vector<float> nodes;
    std::vector<QTask> st;
    uint32_t maxNeed = 0;
    auto alloc = [&]() {
        const uint32_t q = (uint32_t)(nodes.size() / (4 * PG_QNODE_F4));
        nodes.resize(nodes.size() + 4 * PG_QNODE_F4, 0.0f);
        return q;
    };
    out.top_nodes = 0;  // set below: the 4-wide nodes of the breadth-first top levels
    if (bn[0].leaf) {  // the root is a leaf: one node with one leaf slot
        out.top_nodes = 1;
        const uint32_t q = alloc();
        float *o = &nodes[(size_t)q * 4 * PG_QNODE_F4];
        int32_t r[4] = {ref(0, 0), PG_QNODE_EMPTY, PG_QNODE_EMPTY, PG_QNODE_EMPTY};
        float box[6][4] = {};
        for (int a = 0; a < 3; ++a) {
            box[2 * a][0] = bn[0].box.lo[a];
            box[2 * a + 1][0] = bn[0].box.hi[a];
        }
        putQuadNode(o, box, r, 1);
        out.nodes.swap(nodes);
        return true;
    }
    // the top PG_BVH4_TOP_LEVELS levels' nodes are processed breadth first, so their children -- the
    // nodes of depths <= PG_BVH4_TOP_LEVELS -- take the first indices; the rest depth
    // first.  Node contents and refs do not depend on the order: walks return the same hits.
    std::vector<QTask> bfs{{0, alloc(), 1}};
    std::vector<uint32_t> depthOf{0};
    size_t head = 0;
    auto depth = [&](uint32_t q) { return q < depthOf.size() ? depthOf[q] : 0xFFFFFFFFu; };
    while (true) {
        QTask t;
        if (head < bfs.size()) {
            t = bfs[head++];
        } else if (!st.empty()) {
            t = st.back();
            st.pop_back();
        } else {
            break;
        }
        const uint32_t td = depth(t.qnode);
        std::vector<int32_t> ch;
        if (!greedy) collect(t.bnode, ch);
        else ch = {bn[t.bnode].child[0], bn[t.bnode].child[1]};
        while (greedy && ch.size() < 4) {
            int best = -1;
            float bestA = -1.0f;
            for (size_t i = 0; i < ch.size(); ++i)
                if (!bn[ch[i]].leaf && bn[ch[i]].box.area() > bestA) {
                    bestA = bn[ch[i]].box.area();
                    best = (int)i;
                }
            if (best < 0) break;
            const int32_t m = ch[best];
            ch[best] = bn[m].child[0];
            ch.insert(ch.begin() + best + 1, bn[m].child[1]);
        }
        const uint32_t need = t.stackNeed + (uint32_t)ch.size() - 1;
        maxNeed = std::max(maxNeed, need);
        int32_t r[4] = {PG_QNODE_EMPTY, PG_QNODE_EMPTY, PG_QNODE_EMPTY, PG_QNODE_EMPTY};
        float box[6][4];
        for (int a = 0; a < 6; ++a)
            for (int s = 0; s < 4; ++s) box[a][s] = 0.0f;
        for (size_t s = 0; s < ch.size(); ++s) {
            const BNode &c = bn[ch[s]];
            for (int a = 0; a < 3; ++a) {
                box[2 * a][s] = c.box.lo[a];
                box[2 * a + 1][s] = c.box.hi[a];
            }
            if (c.leaf) {
                r[s] = ref(ch[s], 0);
            } else {
                const uint32_t q = alloc();
                r[s] = (int32_t)q;
                if (td != 0xFFFFFFFFu && td + 1 < (uint32_t)PG_BVH4_TOP_LEVELS) {  // breadth-first top levels
                    depthOf.resize(q + 1, 0xFFFFFFFFu);
                    depthOf[q] = td + 1;
                    bfs.push_back({ch[s], q, need});
                } else {
                    st.push_back({ch[s], q, need});
                }
            }
        }
        float *o = &nodes[(size_t)t.qnode * 4 * PG_QNODE_F4];
        putQuadNode(o, box, r, (int)ch.size());
        if (head == bfs.size() && out.top_nodes == 0) out.top_nodes = (uint32_t)(nodes.size() / (4 * PG_QNODE_F4));
    }
    out.nodes.swap(nodes);
    return maxNeed <= PG_QSTACK_DEPTH;
}

bool buildBvh(const float *P, const uint32_t *I, uint32_t nt, uint32_t stack_limit, BvhOut &out) {
    if (nt == 0) {  // every ray misses: a 4-wide node without children; a childless wide node
        out.nodes.assign(4 * PG_QNODE_F4, 0.0f);
        const int32_t r[4] = {PG_QNODE_EMPTY, PG_QNODE_EMPTY, PG_QNODE_EMPTY, PG_QNODE_EMPTY};
        const float box[6][4] = {};
        putQuadNode(out.nodes.data(), box, r, 0);
        out.wnodes.assign(PG_WIDE_NODE_F4 * 4, 0.0f);
        out.order.clear();
        out.tris.clear();
        out.max_depth = out.wide_depth = 1;
        out.top_nodes = 1;
        for (int a = 0; a < 3; ++a) out.lo[a] = out.hi[a] = 0.0f;
        return true;
    }
    // one binary build (leaves <= PG_WIDE_LEAF_MAX triangles) serves both BVHs, and both walk one
    // triangle array in one order (the L2 of an XCD then holds one copy of the triangles)
    std::vector<BNode> bn;
    std::vector<uint32_t> ord, posOf;
    uint32_t maxDepth = 0;
    Box all;
    buildBinary(P, I, nt, PG_WIDE_LEAF_MAX, bn, ord, maxDepth, all);
    for (int a = 0; a < 3; ++a) {
        out.lo[a] = all.lo[a];
        out.hi[a] = all.hi[a];
    }
    auto collapse = [&](const std::vector<BNode> &b, const std::vector<uint32_t> &o, uint32_t depth) {
        out.sah_cost = sahCost(b);
        if (!buildWide(P, I, nt, stack_limit, b, o, out, posOf)) return false;
        out.max_depth = depth;
        return buildQuadBvh(b, posOf, out);
    };
    const int mode = reinsertMode();
    if (mode != 0 && bn.size() > 3) {
        // The collapses below address nodes only through child[] from node 0 and assume nothing about the order
        // of node indices, so the node array stays as the moves leave it.  They do assume that a subtree's
        // triangles are one range of `ord` starting at its leftmost leaf's `first` (rFirst / rCount, posOf): the
        // order is emitted again, depth first.
        std::vector<BNode> bn2 = bn;
        std::vector<uint32_t> ord2 = ord;
        uint32_t depth2 = 0;
        Reinserter r(bn2, std::max(maxDepth, 40u));
        r.run(kReinsertSweeps);
        emitDepthFirst(bn2, ord2, depth2);
        // the pass is an optimisation: a tree a collapse refuses (stack bounds) is dropped for the one it came from
        if (mode != 2 && collapse(bn2, ord2, depth2)) return true;
    }
    return collapse(bn, ord, maxDepth);
}

}  // namespace pgh
