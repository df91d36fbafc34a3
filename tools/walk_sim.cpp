// CPU model of the two walk strategies on the real scene (development tool).
//
//   link walk   the reference's stackless traversal (ray_query.hh:184-278)
//               with the paired-record step of the TravRec walker (one
//               64 B record = a node and the node its `cancel` names)
//   block walk  child-block records + a per-lane stack (device/block_format.h)
//
// Both run on the same rays with the same arithmetic; the tool checks that
// every query returns the same hit bits and prints per-query step and byte
// counts and the block walk's stack depth.  Rays: pinhole camera rays of a
// frame, their closest hits, then up to four random bounces per path plus a
// shadow ray toward the sun from every hit (the wavefront's query mix).
//
//   make -C tools walk_sim && tools/_bin/walk_sim <assets> <frame> [paths] [ring dwords]
//
// Environment switches (each a model experiment):
//   AXIS=1        bounces with zero / NaN direction components in the mix
//   CLOSEBOUND=1  closest-hit walks started with tmax just above their own hit
//   OCC=1, ANYORDER, CLOSEORDER, ORDERLEVEL, LOCKSTEP, CACHESIM, PACKET, SPEC,
//   NONEAR, SCHED   (see their blocks below)
//   ANYHIER=c     (walk_simh build) any-hit walks also over BLASes rebuilt with
//                 SAH traversal cost c (the same triangle leaves and leaf boxes;
//                 the any-hit result is the OR over leaves, so only the leaf
//                 boxes must be the reference's): same results, step counts
// It also prints the share of the mix's shadow rays whose sun ray is blocked
// by the ground (the surface pass leaves those untraced, nee_shadow_moot).
#include "ptg.h"
#include "../path-tracing...but-on-the-lumi-cluster_amd/csrc/host/block_bvh.h"
#include "../path-tracing...but-on-the-lumi-cluster_amd/csrc/host/hmath.h"
#ifdef PTG_MODEL_HOOKS
#include "../path-tracing...but-on-the-lumi-cluster_amd/csrc/host/scene_internal.h"
#endif
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <vector>

using namespace ptg;
using namespace ptg::hm;

namespace {

struct Query { f3 o, d; float tmin, tmax; uint32_t subframe; bool any; uint32_t round = 0; uint32_t src = 0; };
struct Res {
    float t = -1.0f, u = 0, v = 0;
    uint32_t inst = 0xFFFFFFFFu, prim = 0;
    bool back = false, occluded = false;
    uint32_t occ_inst = 0xFFFFFFFFu, occ_prim = 0;   // any hit: the accepted triangle (not compared)
    bool operator==(const Res& r) const
    {
        return memcmp(&t, &r.t, 4) == 0 && memcmp(&u, &r.u, 4) == 0 && memcmp(&v, &r.v, 4) == 0 && inst == r.inst &&
               prim == r.prim && back == r.back && occluded == r.occluded;
    }
};
struct Stats {
    double queries = 0, visits = 0, steps = 0, dep_loads = 0, bytes = 0, tri = 0, enters = 0;
    double block_steps = 0, leaf_steps = 0, pushes = 0, pops = 0, spills = 0, culled = 0, iters = 0;
    std::map<uint32_t, uint64_t> depth_hist;
};

float srcp(float d) { return d == 0 ? (float)1e40 : 1.0f / d; }
uint32_t octant(f3 d) { return (d.x > 0 ? 1u : 0u) | (d.y > 0 ? 2u : 0u) | (d.z > 0 ? 4u : 0u); }

bool box(f3 org, f3 inv, float tmin, float tmax, const float lo[3], const float hi[3], float& nearv)
{
    const float t0x = (lo[0] - org.x) * inv.x, t1x = (hi[0] - org.x) * inv.x;
    const float t0y = (lo[1] - org.y) * inv.y, t1y = (hi[1] - org.y) * inv.y;
    const float t0z = (lo[2] - org.z) * inv.z, t1z = (hi[2] - org.z) * inv.z;
    nearv = fmaxf_(fminf_(t0x, t1x), fmaxf_(fminf_(t0y, t1y), fminf_(t0z, t1z)));
    const float farv = fminf_(fmaxf_(t0x, t1x), fminf_(fmaxf_(t0y, t1y), fmaxf_(t0z, t1z)));
    return nearv <= farv && farv > tmin && nearv < tmax;
}

struct Blas { f3 org, inv, S, bd; int axis; const ptg_tlas_instance* in; uint32_t id; };

Blas enter(const ptg_tlas_instance& in, uint32_t id, f3 o, f3 d)
{
    Blas b;
    b.in = &in;
    b.id = id;
    f4 oo = mul_m4v4(in.inv_transform, v4(o.x, o.y, o.z, 1));
    b.org = v3(oo.x, oo.y, oo.z);
    b.bd = mul_m3v3(extract(in.inv_transform), d);
    b.inv = v3(srcp(b.bd.x), srcp(b.bd.y), srcp(b.bd.z));
    const f3 dd = b.bd;
    f3 ad = v3(std::fabs(dd.x), std::fabs(dd.y), std::fabs(dd.z)), rd = dd;
    b.axis = 2;
    if(ad.x > ad.y && ad.x > ad.z) { b.axis = 0; rd = v3(dd.z, dd.y, dd.x); }
    else if(ad.y > ad.z) { b.axis = 1; rd = v3(dd.x, dd.z, dd.y); }
    b.S = v3(rd.x, rd.y, 1.0f) * (1.0f / rd.z);
    return b;
}

// ray_triangle_intersection + distance test; true = accepted candidate
bool tri(const Blas& b, const ptg_scene_view& v, uint32_t prim, float tmin, float tmax, Res& c)
{
    const uint32_t* t = v.indices + b.in->m.index_offset + size_t(prim) * 3;
    const ptg_float3* P = v.pos + b.in->m.base_vertex_offset;
    f3 A = P[t[0]] - b.org, B = P[t[1]] - b.org, C = P[t[2]] - b.org;
    f3 x = v3(A.x, B.x, C.x), y = v3(A.y, B.y, C.y), z = v3(A.z, B.z, C.z);
    if(b.axis == 0) { x = z; z = v3(A.x, B.x, C.x); }
    else if(b.axis == 1) { y = z; z = v3(A.y, B.y, C.y); }
    x = x - b.S.x * z;
    y = y - b.S.y * z;
    f3 uvw = cross(y, x);
    float det = uvw.x + uvw.y + uvw.z;
    f3 uvt = v3(uvw.x, uvw.y, dot(uvw, b.S.z * z)) * (1.0f / det);
    bool back = det < 0;
    if(b.S.z < 0) back = !back;
    if(b.axis != 2) back = !back;
    bool hit = det != 0.0f && uvt.z >= 0.0f &&
               ((uvw.x >= 0.0f && uvw.y >= 0.0f && uvw.z >= 0.0f) || (uvw.x <= 0.0f && uvw.y <= 0.0f && uvw.z <= 0.0f));
    if(!(hit && uvt.z < tmax && uvt.z > tmin)) return false;
    c.t = uvt.z; c.u = uvt.x; c.v = uvt.y; c.back = back; c.inst = b.id; c.prim = prim;
    return true;
}

// ---- link walk (paired records) ----------------------------------------------
Res link_walk(const ptg_scene_view& v, const Query& q, Stats& st)
{
    const ptg_bvh tl = v.subframes[q.subframe].tlas;
    Res best;
    float tmax = q.tmax;
    f3 org = q.o, inv = v3(srcp(q.d.x), srcp(q.d.y), srcp(q.d.z));
    const f3 winv = inv;
    ptg_bvh as = tl;
    uint32_t lo = tl.node_offset * 8 + octant(q.d) * tl.node_count, node = 0, tres = 0;
    bool in_blas = false;
    Blas b{};
    st.queries++;
    for(;;)
    {
        if(node >= as.node_count)
        {
            st.steps++;
            if(!in_blas) break;
            in_blas = false; as = tl; org = q.o; inv = winv; node = tres;
            lo = tl.node_offset * 8 + octant(q.d) * tl.node_count;
            continue;
        }
        st.steps++;
        st.bytes += 64;
        uint32_t n = node;
        float nv;
        const ptg_bvh_node* N = v.nodes + as.node_offset;
        const ptg_bvh_link* K = v.links + lo;
        st.visits++;
        if(!box(org, inv, q.tmin, tmax, &N[n].min_x, &N[n].max_x, nv))
        {
            const uint32_t c = K[n].cancel;
            if(c >= as.node_count) { node = c; continue; }
            st.visits++;
            n = c;
            if(!box(org, inv, q.tmin, tmax, &N[n].min_x, &N[n].max_x, nv)) { node = K[n].cancel; continue; }
        }
        const uint32_t a = K[n].accept;
        if(!(a & 0x80000000u)) { node = a; continue; }
        node = K[n].cancel;
        const uint32_t leaf = a & 0x7FFFFFFFu;
        st.dep_loads++;
        if(!in_blas)
        {
            st.enters++;
            st.bytes += 64;
            tres = node;
            const ptg_tlas_instance& in = v.instances[leaf];
            b = enter(in, leaf, q.o, q.d);
            in_blas = true; as = in.blas; org = b.org; inv = b.inv; node = 0;
            lo = as.node_offset * 8 + octant(b.bd) * as.node_count;
            continue;
        }
        st.tri++;
        st.bytes += 48;
        Res c;
        if(tri(b, v, leaf, q.tmin, tmax, c))
        {
            if(q.any) { best.occluded = true; return best; }
            best = c;
            tmax = c.t;
        }
    }
    return best;
}

constexpr uint32_t POP = 0xFFFFFFFFu;
double g_last_split[3];   // block_walk: TLAS block steps, steps in the last BLAS, BLAS entries (OCC model)

// ---- block walk (production packer, device algorithm) -----------------------
bool g_spec = true;   // SPEC=0: no parked triangles
std::set<uint64_t>* g_visits = nullptr;   // PACKET=1: the (instance, block) pairs a query steps
uint64_t g_last_block = ~0ull;              // the (instance, block) pair the last node step stepped
std::vector<uint64_t>* g_lines = nullptr;  // CACHESIM: the 128-byte lines a step reads

struct Packed {
    std::vector<BlockCopy> E;          // the device block buffer: [BLAS blocks][TLAS blocks]
    std::vector<uint8_t> order_axes;   // per block: the axes whose sign changes its entry order (COPIES=v model)
    std::vector<uint32_t> inst_root;   // per instance: BLAS root block
    std::vector<uint32_t> tlas_root;   // per subframe
};

// The device walker (path_tracer.h BlockWalker) step for step: node steps
// (pop + block) and leaf steps (parked triangle / BLAS entry / triangle),
// scheduled as the wavefront walk kernel does (U node phases, one leaf phase).
struct SimWalker {
    const ptg_scene_view& v;
    const Packed& pk;
    const Query& q;
    Stats& st;
    uint32_t C;                                         // LDS ring entries (spill counting)
    std::vector<std::pair<uint32_t, uint32_t>> stack;   // (word, near bits)
    uint32_t bsp = 0, cur, pend = kBePop, maxd = 0;
    float tmax, cnear = -INFINITY, pnear = 0;
    f3 org, dir, inv, winv;
    int axis = -1;
    Blas b{};
    Res best;
    bool spec;
    uint32_t skip = 0xFFFFFFFFu;   // OCC model: an instance not to enter (walked first already)
    double tl_steps = 0, blas_cur = 0, enters_n = 0;   // OCC model: TLAS block steps, steps in the current BLAS, entries
    double first_confirm_steps = -1;                     // FIRSTHIT model: st.steps when the first hit was confirmed

    SimWalker(const ptg_scene_view& v_, const Packed& pk_, const Query& q_, Stats& st_, uint32_t C_, bool spec_)
        : v(v_), pk(pk_), q(q_), st(st_), C(C_), spec(spec_)
    {
        tmax = q.tmax;
        org = q.o; dir = q.d;
        inv = winv = v3(srcp(q.d.x), srcp(q.d.y), srcp(q.d.z));
        cur = pk.tlas_root[q.subframe];
    }
    bool at_leaf() const { return (cur & kBeLeaf) && cur != kBePop; }
    bool wants_leaf() const { return pend != kBePop || at_leaf(); }
    void park()
    {
        if(spec && axis >= 0 && pend == kBePop && at_leaf()) { pend = cur; pnear = cnear; cur = kBePop; }
    }
    void push(uint32_t w, float n)
    {
        uint32_t nb;
        memcpy(&nb, &n, 4);
        stack.push_back({w, nb});
        st.pushes++;
        if(stack.size() > C) st.spills++;
        maxd = std::max<uint32_t>(maxd, uint32_t(stack.size()));
    }
    int node_step()
    {
        if(cur == kBePop)
        {
            for(;;)
            {
                if(stack.size() == (axis < 0 ? 0u : bsp))
                {
                    if(axis < 0) return 1;
                    if(pend != kBePop) return 0;
                    axis = -1; org = q.o; dir = q.d; inv = winv;
                    continue;
                }
                const auto e = stack.back();
                stack.pop_back();
                st.pops++;
                float n;
                memcpy(&n, &e.second, 4);
                if(n < tmax) { cur = e.first; cnear = n; break; }
            }
            if(cur & kBeLeaf) { park(); return 0; }
        }
        return block_step();
    }
    // The device's node phase (path_tracer.h node_pop + node_block) with up
    // to K pops: K = 1 is the shipped kernel (a culled entry or a parked
    // triangle costs the lane its phase).  `loaded`: the phase read a block.
    int dev_node_phase(int K, bool& loaded)
    {
        loaded = false;
        for(int k = 0; k < K && cur == kBePop; ++k)
        {
            if(stack.size() == (axis < 0 ? 0u : bsp))
            {
                if(axis < 0) return 1;
                if(pend != kBePop) return 0;
                axis = -1; org = q.o; dir = q.d; inv = winv;
                if(stack.empty()) return 1;
            }
            const auto e = stack.back();
            stack.pop_back();
            st.pops++;
            float n;
            memcpy(&n, &e.second, 4);
            static const bool nonear = getenv("NONEAR") != nullptr;   // 4-byte entries: blocks popped without their near test
            if(!(n < tmax) && !(nonear && !(e.first & kBeLeaf))) continue;
            cur = e.first;
            cnear = n;
            if(cur & kBeLeaf)
            {
                park();
                if(at_leaf()) return 0;
            }
        }
        if(cur == kBePop || at_leaf()) return 0;
        loaded = true;
        return block_step();
    }
    int block_step()
    {
        if(axis < 0) tl_steps++;
        else blas_cur++;
        st.steps++;
        st.block_steps++;
        st.bytes += 128;
        if(g_visits) g_visits->insert((uint64_t(axis < 0 ? 0xFFFFFFFFu : b.id) << 32) | cur);
        g_last_block = (uint64_t(axis < 0 ? 0xFFFFFFFFu : b.id) << 32) | cur;
        // the ray octant's copy: entries in the ray's order, boxes as (near, far) planes
        const BlockCopy& bc = pk.E[size_t(cur) * kBlockCopies + octant(dir)];
        if(g_lines)
        {   // the copy's 128 B lines.  COPIES (model only):
            // 8 = one copy per ray octant (the shipped layout); 2 = one per sign
            // of the ray's x direction; 1 = a single copy per block (its order
            // for the ray's octant from an order word in the same line)
            static const uint32_t copies = getenv("COPIES") ? uint32_t(atoi(getenv("COPIES"))) : kBlockCopies;
            // COPIES=0: one copy per distinct entry order of the block (its
            // order depends only on the signs of the axes in order_axes):
            // copy (octant & mask), 2^popcount(mask) lines per block
            const uint32_t sub = copies == 8 ? octant(dir) : copies == 2 ? (dir.x > 0 ? 1u : 0u)
                                 : copies == 4 ? (octant(dir) & 3u)
                                 : copies == 0 ? (octant(dir) & pk.order_axes[cur]) : 0u;
            const size_t span = copies == 0 ? 8u : copies;
            for(size_t k = 0; k < sizeof(BlockCopy) / 128; ++k)
                g_lines->push_back((size_t(cur) * span + sub) * (sizeof(BlockCopy) / 128) + k);
        }
        const bool fin = std::isfinite(inv.x) && std::isfinite(inv.y) && std::isfinite(inv.z);
        uint32_t cand = kBePop;
        float cn = 0;
        // ORDER experiments (model only): 0 = the stored octant order (the
        // reference's); 1 = nearest entry first; 2 = reversed; 3 = largest box
        // first.  ANYORDER applies to any-hit queries, CLOSEORDER to closest-hit.
        static const int any_order = getenv("ANYORDER") ? atoi(getenv("ANYORDER")) : 0;
        static const int close_order = getenv("CLOSEORDER") ? atoi(getenv("CLOSEORDER")) : 0;
        static const int order_level = getenv("ORDERLEVEL") ? atoi(getenv("ORDERLEVEL")) : 0;   // 0 both, 1 TLAS only, 2 BLAS only
        int order = q.any ? any_order : close_order;
        if((order_level == 1 && axis >= 0) || (order_level == 2 && axis < 0)) order = 0;
        if(order)
        {
            struct E { uint32_t a; float n, key; };
            E es[kBlockWidth];
            int ne = 0;
            for(uint32_t j = 0; j < kBlockWidth; ++j)
            {
                const BlockCopy::Near& x = bc.n[j];
                const float* xf = &bc.f[3 * j];
                if(x.a & kBeNone) continue;
                float n;
                st.visits++;
                if(!box(org, inv, q.tmin, tmax, &x.x, xf, n)) continue;
                float key = float(j);
                if(order == 1) key = n;
                else if(order == 2) key = -float(j);
                else if(order == 3)
                {
                    const float dx = std::fabs(xf[0] - x.x), dy = std::fabs(xf[1] - x.y), dz = std::fabs(xf[2] - x.z);
                    key = -(dx * dy + dy * dz + dz * dx);
                }
                es[ne++] = E{x.a, n, key};
            }
            std::stable_sort(es, es + ne, [](const E& a, const E& b) { return a.key < b.key; });
            for(int k = ne - 1; k >= 1; --k) push(es[k].a, es[k].n);
            cur = ne ? es[0].a : kBePop;
            cnear = ne ? es[0].n : 0.0f;
            park();
            return 0;
        }
        for(int j = int(kBlockWidth) - 1; j >= 0; --j)
        {
            const BlockCopy::Near& x = bc.n[j];
            const float* xf = &bc.f[3 * j];
            if(x.a & kBeNone) continue;
            float n;
            st.visits++;
            bool pass;
            if(fin)
            {   // the device's fast form: near = max of near-plane t, far = min of far-plane t,
                // the interval clamped to [next(tmin), prev(tmax)] (BlockWalker::box_near_far)
                float tmin_p = q.tmin, tmax_m = tmax;
                uint32_t bits;
                memcpy(&bits, &tmin_p, 4); bits += 1; memcpy(&tmin_p, &bits, 4);
                memcpy(&bits, &tmax_m, 4); bits -= 1; memcpy(&tmax_m, &bits, 4);
                const float tnx = (x.x - org.x) * inv.x, tfx = (xf[0] - org.x) * inv.x;
                const float tny = (x.y - org.y) * inv.y, tfy = (xf[1] - org.y) * inv.y;
                const float tnz = (x.z - org.z) * inv.z, tfz = (xf[2] - org.z) * inv.z;
                n = fmaxf_(fmaxf_(tnx, tmin_p), fmaxf_(tny, tnz));
                const float f = fminf_(fminf_(tfx, tmax_m), fminf_(tfy, tfz));
                pass = n <= f;
            }
            else
                pass = box(org, inv, q.tmin, tmax, &x.x, xf, n);
            if(!pass) continue;
            if(cand != kBePop) push(cand, cn);
            cand = x.a;
            cn = n;
        }
        cur = cand;
        cnear = cn;
        park();
        return 0;
    }
    int tri_at(uint32_t id, float n)
    {
        if(!(n < tmax)) return 0;
        blas_cur++;
        st.steps++;
        st.leaf_steps++;
        st.tri++;
        st.bytes += 48;
        if(g_lines) g_lines->push_back((1ull << 40) + (uint64_t(b.in->m.index_offset / 3 + id) * 48) / 128);   // TriRec
        Res c;
        if(tri(b, v, id, q.tmin, tmax, c))
        {
            if(q.any) { best.occluded = true; best.occ_inst = b.id; best.occ_prim = id; return 2; }
            best = c;
            tmax = c.t;
            if(first_confirm_steps < 0) first_confirm_steps = st.steps;
        }
        return 0;
    }
    int leaf_step()
    {
        if(pend != kBePop)
        {
            const uint32_t id = pend & kBeIndex;
            const float n = pnear;
            pend = kBePop;
            if(int r = tri_at(id, n)) return r;
            park();
            return 0;
        }
        const uint32_t id = cur & kBeIndex;
        const float n = cnear;
        cur = kBePop;
        if(axis < 0)
        {
            if(id == skip) return 0;   // OCC model: this instance was walked first
            enters_n++;
            blas_cur = 0;
            st.steps++;
            st.leaf_steps++;
            st.enters++;
            st.bytes += 64;
            if(g_lines) g_lines->push_back((2ull << 40) + id / 2);   // InstTrav, 64 B
            const ptg_tlas_instance& in = v.instances[id];
            b = enter(in, id, q.o, q.d);
            axis = b.axis; bsp = uint32_t(stack.size());
            org = b.org; inv = b.inv; dir = b.bd;
            cur = pk.inst_root[id];
            return 0;
        }
        return tri_at(id, n);
    }
};

double g_max_query_steps = 0;   // the most block-walk steps any query took

Res block_walk(const ptg_scene_view& v, const Packed& pk, const Query& q, Stats& st, uint32_t C)
{
    st.queries++;
    const double steps0 = st.steps;
    SimWalker w(v, pk, q, st, C, g_spec);
    static const int sched = getenv("SCHED") ? atoi(getenv("SCHED")) : 0;
    for(;;)
    {
        int r = 0;
        if(sched == 1)
        {   // experiment: [mixed phase: leaf work if any, else a node step] + [node phase]
            r = w.wants_leaf() ? w.leaf_step() : w.node_step();
            if(r == 0 && !w.at_leaf()) r = w.node_step();
        }
        else
        {
            for(int u = 0; u < 2 && r == 0; ++u)
                if(!w.at_leaf()) r = w.node_step();
            if(r == 0 && w.wants_leaf()) r = w.leaf_step();
        }
        if(r) break;
        st.iters++;
    }
    st.depth_hist[w.maxd]++;
    g_max_query_steps = std::max(g_max_query_steps, st.steps - steps0);
    if(getenv("FIRSTHIT") && !q.any)
    {   // model: a closest-hit walk that may stop at its first confirmed hit
        // (the last bounce when no emissive instance can be hit): steps to that
        // hit against the whole walk, for bounce rays (round >= 1)
        static double all = 0, upto = 0, n = 0, nh = 0;
        if(q.round >= 1)
        {
            all += st.steps - steps0;
            upto += w.first_confirm_steps >= 0 ? w.first_confirm_steps - steps0 : st.steps - steps0;
            n += 1;
            nh += w.first_confirm_steps >= 0;
            if(uint64_t(n) % 20000 == 0)
                fprintf(stderr, "FIRSTHIT: %.0f bounce queries (%.1f%% hit): steps %.2f, to the first confirm %.2f (%.1f%%)\n", n,
                        100 * nh / n, all / n, upto / n, 100 * upto / all);
        }
    }
    g_last_split[0] = w.tl_steps;
    g_last_split[1] = w.blas_cur;
    g_last_split[2] = w.enters_n;
    return w.best;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
float rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return float(rng_state >> 40) / float(1u << 24);
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 3) { fprintf(stderr, "usage: walk_sim <assets> <frame> [paths] [stack] [W]\n"); return 2; }
    const uint32_t frame = uint32_t(atoi(argv[2]));
    const uint32_t paths = argc > 3 ? uint32_t(atoi(argv[3])) : 20000;
    const uint32_t S = argc > 4 ? uint32_t(atoi(argv[4])) : 16;
    if(const char* e = getenv("SPEC")) g_spec = atoi(e) != 0;
    ptg_render_config cfg;
    ptg_render_config_default(&cfg);
    cfg.width = 1280; cfg.height = 720; cfg.samples_per_pixel = 1024;
    ptg_scene* scene = nullptr;
    if(ptg_scene_load(argv[1], &cfg, &scene) || ptg_scene_setup_frame(scene, frame)) { fprintf(stderr, "%s\n", ptg_last_error()); return 1; }
    ptg_scene_view v;
    ptg_scene_view_get(scene, &v);

    // the upload's own packing (BlockCache, as ptg_upload_frame runs it):
    // frame 0 first and committed, so that the frame under test also packs
    // BLASes at a nonzero block base, as a later frame upload does
    BlockCache cache;
    cache.set_scene(v.nodes, v.links, v.static_node_count, v.indices, v.index_count, v.pos, v.albedo, v.material,
                    v.vertex_count);
    FramePack fp;
    std::string err;
    auto pack = [&]() {
        ptg_scene_view w;
        ptg_scene_view_get(scene, &w);
        return cache.pack_frame(w.subframes, w.subframe_count, w.instances, w.instance_count, w.nodes + w.static_node_count,
                                w.links + 8 * w.static_node_count, w.static_node_count, w.node_count - w.static_node_count, fp,
                                err);
    };
    if(frame != 0)
    {
        if(ptg_scene_setup_frame(scene, 0) || pack()) { fprintf(stderr, "frame 0: %s\n", err.c_str()); return 1; }
        cache.commit(fp);
        if(ptg_scene_setup_frame(scene, frame)) { fprintf(stderr, "%s\n", ptg_last_error()); return 1; }
        ptg_scene_view_get(scene, &v);
    }
    const auto tp0 = std::chrono::steady_clock::now();
    if(pack()) { fprintf(stderr, "frame %u: %s\n", frame, err.c_str()); return 1; }
    printf("pack_frame %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count());
    if(getenv("PACKTIME"))
    {   // steady state: the same frame again with its BLASes committed (TLASes only)
        FramePack keep = fp;
        cache.commit(fp);
        for(int k = 0; k < 3; ++k)
        {
            const auto t1 = std::chrono::steady_clock::now();
            if(pack()) return 1;
            printf("pack_frame again %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
        }
        return 0;
    }
    Packed pk;
    pk.E = cache.blas;
    pk.E.insert(pk.E.end(), fp.new_blas.begin(), fp.new_blas.end());
    pk.E.insert(pk.E.end(), fp.tlas.begin(), fp.tlas.end());
    {   // per block: the axes a whose sign flip changes some octant's entry order
        const size_t nb = pk.E.size() / kBlockCopies;
        pk.order_axes.assign(nb, 0);
        double lines = 0;
        size_t hist[8] = {};
        for(size_t k = 0; k < nb; ++k)
        {
            uint8_t m = 0;
            for(uint32_t o = 0; o < 8; ++o)
                for(uint32_t a = 0; a < 3; ++a)
                    for(uint32_t j = 0; j < kBlockWidth; ++j)
                        if(pk.E[k * 8 + o].n[j].a != pk.E[k * 8 + (o ^ (1u << a))].n[j].a) m |= uint8_t(1u << a);
            pk.order_axes[k] = m;
            lines += double(1u << __builtin_popcount(m));
            hist[m]++;
        }
        printf("blocks %zu: distinct orders per block %.2f on average; axis masks", nb, lines / double(nb));
        for(int m = 0; m < 8; ++m) printf(" %d:%zu", m, hist[m]);
        printf("\n");
    }
    pk.inst_root = fp.inst_root;
    pk.tlas_root = fp.tlas_root;
    {   // the any-hit candidates' requirement (pack_frame checks it per BLAS and mesh:
        // an instance that fails it offers no candidate triangles)
        ptg_scene_view w;
        ptg_scene_view_get(scene, &w);
        size_t bad = 0;
        for(size_t i = 0; i < w.instance_count; ++i) bad += fp.inst_box[i].tri_count != 0 ? 0 : 1;
        printf("instances whose BLAS leaf boxes are not their vertex bounds: %zu of %zu\n", bad, w.instance_count);
        {   // and the check rejects a box that is not: instance 0's BLAS with one leaf box's
            // min_x lowered by one ulp, and with +0 / -0 swapped in a zero bound if it has one
            const ptg_tlas_instance& in = w.instances[0];
            std::vector<ptg_bvh_node> nodes(w.nodes + in.blas.node_offset, w.nodes + in.blas.node_offset + in.blas.node_count);
            const ptg_bvh_link* links = w.links + size_t(in.blas.node_offset) * 8;
            uint32_t leaf = 0;
            while(leaf < in.blas.node_count && !(links[leaf].accept & 0x80000000u)) ++leaf;
            bool rejects = leaf < in.blas.node_count;
            if(rejects)
            {
                nodes[leaf].min_x = std::nextafter(nodes[leaf].min_x, -INFINITY);
                rejects = !leaf_boxes_are_vertex_bounds(nodes.data(), links, in.blas.node_count, w.indices, w.index_count, w.pos,
                                                        w.vertex_count, in.m.index_offset, in.m.triangle_count,
                                                        in.m.base_vertex_offset);
            }
            printf("leaf-box check rejects a perturbed box: %s\n", rejects ? "yes" : "no");
        }
    }
    printf("frame %u: BLAS %zu + %zu new copies (%.1f MB), TLAS %zu copies (%.1f MB); stack bound %u entries (TLAS %u)\n",
           frame, cache.blas.size(), fp.new_blas.size(), (cache.blas.size() + fp.new_blas.size()) * 128 / 1e6, fp.tlas.size(),
           fp.tlas.size() * 128 / 1e6, fp.stack_bound(), fp.tlas_stack);

    if(getenv("PACKET"))
    {   // how much a wave of camera rays (8 pixels x 8 jittered samples, one
        // subframe) shares: the union of the blocks its lanes step
        double lane_steps = 0, union_steps = 0, groups = 0;
        for(int g = 0; g < 400; ++g)
        {
            const uint32_t px0 = uint32_t(rnd() * (cfg.width / 8)) * 8, py = uint32_t(rnd() * cfg.height);
            const uint32_t sf = uint32_t(rnd() * v.subframe_count) % v.subframe_count;
            const ptg_camera& cam = v.subframes[sf].cam;
            std::set<uint64_t> uni;
            for(int l = 0; l < 64; ++l)
            {
                const float fx = px0 + (l >> 3) + rnd(), fy = py + rnd();
                float ux = fx / cfg.width * 2.0f - 1.0f, uy = fy / cfg.height * 2.0f - 1.0f;
                ux *= cam.aspect_ratio;
                uy = -uy;
                f3 d = normalize(v3(ux * cam.inv_focal_length, uy * cam.inv_focal_length, -1.0f));
                d = mul_m3v3(cam.orientation, d);
                std::set<uint64_t> mine;
                g_visits = &mine;
                Stats tmp;
                block_walk(v, pk, Query{cam.position, d, 0.0f, 1e9f, sf, false}, tmp, S);
                g_visits = nullptr;
                lane_steps += double(mine.size());
                uni.insert(mine.begin(), mine.end());
            }
            union_steps += double(uni.size());
            groups += 1;
        }
        printf("camera-ray waves: %.1f block steps per lane, %.1f in the union of a wave's 64 lanes\n", lane_steps / groups / 64,
               union_steps / groups);
        // the device's lockstep schedule (2 node phases, 1 leaf phase) for such waves: how many node
        // phases have every stepping lane on the same block
        double phases = 0, uniform = 0, distinct = 0, iters = 0;
        for(int g = 0; g < 200; ++g)
        {
            const uint32_t px0 = uint32_t(rnd() * (cfg.width / 8)) * 8, py = uint32_t(rnd() * cfg.height);
            const uint32_t sf = uint32_t(rnd() * v.subframe_count) % v.subframe_count;
            const ptg_camera& cam = v.subframes[sf].cam;
            std::vector<Query> wq(64);
            std::vector<Stats> wst(64);
            std::vector<std::unique_ptr<SimWalker>> ws;
            for(int l = 0; l < 64; ++l)
            {
                const float fx = px0 + (l >> 3) + rnd(), fy = py + rnd();
                float ux = fx / cfg.width * 2.0f - 1.0f, uy = fy / cfg.height * 2.0f - 1.0f;
                ux *= cam.aspect_ratio;
                uy = -uy;
                f3 d = normalize(v3(ux * cam.inv_focal_length, uy * cam.inv_focal_length, -1.0f));
                wq[l] = Query{cam.position, mul_m3v3(cam.orientation, d), 0.0f, 1e9f, sf, false};
            }
            for(int l = 0; l < 64; ++l) ws.emplace_back(new SimWalker(v, pk, wq[l], wst[l], S, g_spec));
            std::vector<char> act(64, 1);
            for(;;)
            {
                bool any = false;
                for(int l = 0; l < 64; ++l) any = any || act[l];
                if(!any) break;
                iters++;
                for(int u = 0; u < 2; ++u)
                {
                    std::set<uint64_t> stepped;
                    for(int l = 0; l < 64; ++l)
                    {
                        if(!act[l] || ws[l]->at_leaf()) continue;
                        g_last_block = ~0ull;
                        if(ws[l]->node_step()) act[l] = 0;
                        if(g_last_block != ~0ull) stepped.insert(g_last_block);
                    }
                    if(!stepped.empty())
                    {
                        phases++;
                        distinct += double(stepped.size());
                        if(stepped.size() == 1) uniform++;
                    }
                }
                for(int l = 0; l < 64; ++l)
                    if(act[l] && ws[l]->wants_leaf() && ws[l]->leaf_step()) act[l] = 0;
            }
        }
        printf("lockstep camera-ray waves: %.1f iterations, %.1f node phases with steps, %.1f%% on one block, %.1f blocks per phase\n",
               iters / 200, phases / 200, 100 * uniform / phases, distinct / phases);
        return 0;
    }

    if(getenv("OCC"))
    {   // Any-hit occluder cache model.  trace_shadow_ray (path_tracer.hh:415-427)
        // returns only whether ray_query_proceed found a candidate; with tmax
        // fixed (no confirm) the result is the OR over triangles of "the TLAS
        // leaf box, the BLAS leaf box and the triangle test all pass" (ancestors
        // pass by containment).  So testing ANY candidate (instance, triangle)
        // with exactly those three tests first is exact: an accept means
        // "occluded".  This model measures how often cheap candidates exist and
        // hit, and what the walks they replace cost.
        //   wavefront query mix: waves of 8 pixels x 8 jittered samples (one
        //   subframe), up to 4 bounces, a shadow ray toward the sun (within its
        //   4-degree cone) from every hit lit from the viewer's side.
        const uint32_t nwaves = paths / 64 ? paths / 64 : 1;
        const double cos_cone = std::cos(4.0 * M_PI / 180.0);
        // per subframe: instance -> its TLAS leaf box (the reference's node)
        std::vector<std::map<uint32_t, std::pair<std::array<float, 3>, std::array<float, 3>>>> tleaf(v.subframe_count);
        for(size_t sf = 0; sf < v.subframe_count; ++sf)
        {
            const ptg_bvh tl = v.subframes[sf].tlas;
            const ptg_bvh_node* N = v.nodes + tl.node_offset;
            const ptg_bvh_link* K = v.links + size_t(tl.node_offset) * 8;
            for(uint32_t n = 0; n < tl.node_count; ++n)
                if(K[n].accept & 0x80000000u)
                    tleaf[sf][K[n].accept & 0x7FFFFFFFu] = {{N[n].min_x, N[n].min_y, N[n].min_z}, {N[n].max_x, N[n].max_y, N[n].max_z}};
        }
        uint64_t tests = 0, test_fail_membership = 0, wrong = 0;
        auto cache_test = [&](const Query& q, uint32_t inst, uint32_t prim) -> bool {
            ++tests;
            auto it = tleaf[q.subframe].find(inst);
            if(it == tleaf[q.subframe].end()) { ++test_fail_membership; return false; }
            float nv;
            const f3 winv = v3(srcp(q.d.x), srcp(q.d.y), srcp(q.d.z));
            if(!box(q.o, winv, q.tmin, q.tmax, it->second.first.data(), it->second.second.data(), nv)) return false;
            const ptg_tlas_instance& in = v.instances[inst];
            if(prim >= in.m.triangle_count) return false;
            const Blas b = enter(in, inst, q.o, q.d);
            const uint32_t* t = v.indices + in.m.index_offset + size_t(prim) * 3;
            const ptg_float3* P = v.pos + in.m.base_vertex_offset;
            const ptg_float3 &A = P[t[0]], &B = P[t[1]], &C = P[t[2]];
            // the BLAS leaf's box: fmin / fmax of the triangle's vertices (bvh.cc:243-246)
            const float lo[3] = {fminf_(A.x, fminf_(B.x, C.x)), fminf_(A.y, fminf_(B.y, C.y)), fminf_(A.z, fminf_(B.z, C.z))};
            const float hi[3] = {fmaxf_(A.x, fmaxf_(B.x, C.x)), fmaxf_(A.y, fmaxf_(B.y, C.y)), fmaxf_(A.z, fmaxf_(B.z, C.z))};
            if(!box(b.org, b.inv, q.tmin, q.tmax, lo, hi, nv)) return false;
            Res c;
            return tri(b, v, prim, q.tmin, q.tmax, c);
        };
        // instance-first walk: the TLAS leaf box of `inst`, then its BLAS walked
        // whole (any hit) before the TLAS; on no hit the normal walk follows,
        // skipping `inst` (walking it again cannot accept).  Returns the steps
        // of both parts; `occ` = the result (must equal the reference's).
        auto inst_first = [&](const Query& q, uint32_t inst, bool& occ, uint32_t prim = 0xFFFFFFFFu) -> double {
            Stats st;
            occ = false;
            if(prim != 0xFFFFFFFFu && cache_test(q, inst, prim)) { occ = true; return 2.0; }   // the triangle first
            if(prim != 0xFFFFFFFFu) st.steps += 1;
            auto it = tleaf[q.subframe].find(inst);
            float nv;
            const f3 winv = v3(srcp(q.d.x), srcp(q.d.y), srcp(q.d.z));
            bool entered = false;
            if(it != tleaf[q.subframe].end() &&
               box(q.o, winv, q.tmin, q.tmax, it->second.first.data(), it->second.second.data(), nv))
            {
                entered = true;
                SimWalker w(v, pk, q, st, S, g_spec);
                w.cur = kBeLeaf | inst;
                w.cnear = nv;
                for(;;)
                {
                    int r = 0;
                    for(int u = 0; u < 2 && r == 0; ++u)
                        if(!w.at_leaf()) r = w.node_step();
                    if(r == 0 && w.wants_leaf()) r = w.leaf_step();
                    if(r) { occ = r == 2; break; }
                }
            }
            if(occ) return st.steps + 1;
            SimWalker w(v, pk, q, st, S, g_spec);
            if(entered) w.skip = inst;
            for(;;)
            {
                int r = 0;
                for(int u = 0; u < 2 && r == 0; ++u)
                    if(!w.at_leaf()) r = w.node_step();
                if(r == 0 && w.wants_leaf()) r = w.leaf_step();
                if(r) { occ = r == 2; break; }
            }
            return st.steps + 1;
        };
        struct SQ { Query q; bool occ; uint32_t oi, op; double steps, block; uint32_t pixel; double tl, last, enters; };
        // shadow queries by [round][wave][lane] (absent: subframe == ~0u)
        std::vector<std::vector<SQ>> sq(4, std::vector<SQ>(size_t(nwaves) * 64));
        for(auto& r: sq) for(auto& x: r) x.q.subframe = ~0u;
        const uint32_t row0 = uint32_t(rnd() * (cfg.height - nwaves / 160 - 1));
        for(uint32_t w = 0; w < nwaves; ++w)
        {
            const uint32_t sf = uint32_t(rnd() * v.subframe_count) % v.subframe_count;
            const ptg_camera& cam = v.subframes[sf].cam;
            const f3 L0 = normalize(v.subframes[sf].light.direction);
            for(uint32_t l = 0; l < 64; ++l)
            {
                const uint32_t px = (8 * w + l / 8) % cfg.width, py = row0 + (8 * w + l / 8) / cfg.width;
                float ux = (px + rnd()) / cfg.width * 2.0f - 1.0f, uy = (py + rnd()) / cfg.height * 2.0f - 1.0f;
                ux *= cam.aspect_ratio;
                uy = -uy;
                f3 d = normalize(mul_m3v3(cam.orientation, normalize(v3(ux * cam.inv_focal_length, uy * cam.inv_focal_length, -1.0f))));
                f3 o = cam.position;
                for(uint32_t bnc = 0; bnc < 4; ++bnc)
                {
                    Stats tmp;
                    const Res r = link_walk(v, Query{o, d, bnc ? 1e-4f : 0.0f, 1e9f, sf, false}, tmp);
                    if(r.inst == 0xFFFFFFFFu) break;
                    const ptg_tlas_instance& in = v.instances[r.inst];
                    const uint32_t* t = v.indices + in.m.index_offset + size_t(r.prim) * 3;
                    const ptg_float3* P = v.pos + in.m.base_vertex_offset;
                    const f3 A = v3(P[t[0]].x, P[t[0]].y, P[t[0]].z), B = v3(P[t[1]].x, P[t[1]].y, P[t[1]].z),
                             C = v3(P[t[2]].x, P[t[2]].y, P[t[2]].z);
                    const f3 ng = normalize(mul_m3v3(extract(in.transform), cross(B - A, C - A)));
                    o = o + d * r.t;
                    // a direction in the sun's cone
                    f3 L;
                    {
                        const double z = 1.0 - rnd() * (1.0 - cos_cone), ph = 2 * M_PI * rnd(), rr = std::sqrt(std::max(0.0, 1 - z * z));
                        const f3 up = std::fabs(L0.x) < 0.9f ? v3(1, 0, 0) : v3(0, 1, 0);
                        const f3 T = normalize(cross(up, L0)), Bt = cross(L0, T);
                        L = normalize(T * float(rr * std::cos(ph)) + Bt * float(rr * std::sin(ph)) + L0 * float(z));
                    }
                    if(dot(ng, L) * dot(ng, -d) > 0)   // lit from the viewer's side: the NEE ray is traced
                    {
                        SQ& x = sq[bnc][size_t(w) * 64 + l];
                        x.q = Query{o, L, 1e-4f, 1e9f, sf, true, bnc, r.inst};
                        x.pixel = py * cfg.width + px;
                        Stats st;
                        const Res br = block_walk(v, pk, x.q, st, S);
                        Stats lt;
                        if(!(link_walk(v, x.q, lt) == br)) ++wrong;
                        x.occ = br.occluded;
                        x.oi = br.occ_inst;
                        x.op = br.occ_prim;
                        x.steps = st.steps;
                        x.block = st.block_steps;
                        x.tl = g_last_split[0];
                        x.last = g_last_split[1];
                        x.enters = g_last_split[2];
                    }
                    // next bounce: a random direction on the viewer's side of the surface
                    f3 nd;
                    do { nd = v3(rnd() * 2 - 1, rnd() * 2 - 1, rnd() * 2 - 1); } while(dot(nd, nd) > 1 || dot(nd, nd) < 1e-4f);
                    nd = normalize(nd);
                    if(dot(nd, ng) * dot(-d, ng) < 0) nd = -nd;
                    d = nd;
                }
            }
        }
        // policies: P = the path's previous occluder; W = occluders found by the wave's
        // earlier lanes this round (most recent K); X = the pixel's last occluder at this
        // round (earlier sample groups); N = the previous wave's occluders this round
        const int K = getenv("OCCK") ? atoi(getenv("OCCK")) : 2;
        const char* names[] = {"P (path)", "W (wave, last K)", "X (pixel)", "N (prev wave)", "P+W", "P+W+X"};
        const int NP = 6;
        double tot_q = 0, tot_occ = 0, steps_all = 0, steps_occ = 0, block_all = 0;
        double have[NP] = {}, hit[NP] = {}, saved[NP] = {}, ntest[NP] = {};
        for(int r = 0; r < 4; ++r)
        {
            std::map<uint32_t, std::pair<uint32_t, uint32_t>> pix;
            std::vector<std::pair<uint32_t, uint32_t>> prevwave;
            for(uint32_t w = 0; w < nwaves; ++w)
            {
                std::vector<std::pair<uint32_t, uint32_t>> wave;   // this round's occluders, lane order
                for(uint32_t l = 0; l < 64; ++l)
                {
                    const SQ& x = sq[r][size_t(w) * 64 + l];
                    if(x.q.subframe == ~0u) continue;
                    tot_q++;
                    steps_all += x.steps;
                    block_all += x.block;
                    if(x.occ) { tot_occ++; steps_occ += x.steps; }
                    std::vector<std::pair<uint32_t, uint32_t>> cands[NP];
                    for(int pr = r - 1; pr >= 0; --pr)
                    {
                        const SQ& y = sq[pr][size_t(w) * 64 + l];
                        if(y.q.subframe != ~0u && y.occ) { cands[0].push_back({y.oi, y.op}); break; }
                    }
                    for(int k = int(wave.size()) - 1; k >= 0 && int(wave.size()) - k <= K; --k) cands[1].push_back(wave[k]);
                    if(auto it = pix.find(x.pixel); it != pix.end()) cands[2].push_back(it->second);
                    for(int k = int(prevwave.size()) - 1; k >= 0 && int(prevwave.size()) - k <= K; --k) cands[3].push_back(prevwave[k]);
                    cands[4] = cands[0];
                    cands[4].insert(cands[4].end(), cands[1].begin(), cands[1].end());
                    cands[5] = cands[4];
                    cands[5].insert(cands[5].end(), cands[2].begin(), cands[2].end());
                    for(int pi = 0; pi < NP; ++pi)
                    {
                        // distinct candidates in order
                        std::vector<std::pair<uint32_t, uint32_t>> c;
                        for(auto& e: cands[pi]) if(std::find(c.begin(), c.end(), e) == c.end()) c.push_back(e);
                        if(c.empty()) continue;
                        have[pi]++;
                        bool ok = false;
                        for(auto& e: c)
                        {
                            ntest[pi]++;
                            if(cache_test(x.q, e.first, e.second)) { ok = true; break; }
                        }
                        if(ok)
                        {
                            if(!x.occ) ++wrong;   // an accepted candidate must mean "occluded"
                            hit[pi]++;
                            saved[pi] += x.steps;
                        }
                    }
                    if(x.occ)
                    {
                        wave.push_back({x.oi, x.op});
                        pix[x.pixel] = {x.oi, x.op};
                    }
                }
                prevwave = wave;
            }
        }
        {
            double a[2][5] = {};
            for(auto& rr: sq)
                for(auto& x: rr)
                    if(x.q.subframe != ~0u)
                    {
                        double* t = a[x.occ ? 1 : 0];
                        t[0]++; t[1] += x.steps; t[2] += x.tl; t[3] += x.last; t[4] += x.enters;
                    }
            for(int k = 0; k < 2; ++k)
                printf("%s queries: %.0f, steps %.2f = TLAS blocks %.2f + BLAS entries %.2f + steps in BLASes %.2f, of which "
                       "the last BLAS %.2f\n", k ? "occluded" : "unoccluded", a[k][0], a[k][1] / a[k][0], a[k][2] / a[k][0],
                       a[k][4] / a[k][0], (a[k][1] - a[k][2] - a[k][4]) / a[k][0], a[k][3] / a[k][0]);
        }
        printf("occluder model, frame %u: %.0f shadow queries (%.1f per path), %.1f%% occluded; block-walk steps per query %.2f "
               "(block %.2f); occluded queries carry %.1f%% of the steps\n",
               frame, tot_q, tot_q / (nwaves * 64.0), 100 * tot_occ / tot_q, steps_all / tot_q, block_all / tot_q,
               100 * steps_occ / steps_all);
        for(int pi = 0; pi < NP; ++pi)
            printf("  %-18s candidate for %5.1f%% of queries, hits %5.1f%% of occluded queries, %.2f tests per query with one; "
                   "steps saved %5.1f%% (net of 1 step per test: %5.1f%%)\n",
                   names[pi], 100 * have[pi] / tot_q, 100 * hit[pi] / std::max(1.0, tot_occ), ntest[pi] / std::max(1.0, have[pi]),
                   100 * saved[pi] / steps_all, 100 * (saved[pi] - ntest[pi]) / steps_all);
        // instance level: the candidate instance's BLAS walked first
        {
            const char* in_names[] = {"Pi (path)", "Wi (wave, last)", "Xi (pixel)", "Pi else Wi", "Pi else Xi else Wi",
                                      "(P else W) tri+inst", "(W) tri+inst", "(G prev group) tri+inst"};
            const int NI = 8;
            double cost[NI] = {}, have_i[NI] = {}, hit_i[NI] = {};
            for(int r = 0; r < 4; ++r)
            {
                std::map<uint32_t, uint32_t> pix;
                uint32_t group_last = 0xFFFFFFFFu, group_last_p = 0xFFFFFFFFu;   // the previous group's last occluder
                for(uint32_t w = 0; w < nwaves; ++w)
                {
                    uint32_t wave_last = 0xFFFFFFFFu, wave_last_p = 0xFFFFFFFFu;
                    const uint32_t prev_g = group_last, prev_gp = group_last_p;
                    for(uint32_t l = 0; l < 64; ++l)
                    {
                        const SQ& x = sq[r][size_t(w) * 64 + l];
                        if(x.q.subframe == ~0u) continue;
                        uint32_t pc = 0xFFFFFFFFu, pp = 0xFFFFFFFFu, xc = 0xFFFFFFFFu;
                        for(int pr = r - 1; pr >= 0; --pr)
                        {
                            const SQ& y = sq[pr][size_t(w) * 64 + l];
                            if(y.q.subframe != ~0u && y.occ) { pc = y.oi; pp = y.op; break; }
                        }
                        if(auto it = pix.find(x.pixel); it != pix.end()) xc = it->second;
                        const uint32_t cand[NI] = {pc, wave_last, xc, pc != ~0u ? pc : wave_last,
                                                   pc != ~0u ? pc : (xc != ~0u ? xc : wave_last),
                                                   pc != ~0u ? pc : wave_last, wave_last, prev_g};
                        const uint32_t cprim[NI] = {~0u, ~0u, ~0u, ~0u, ~0u, pc != ~0u ? pp : wave_last_p, wave_last_p, prev_gp};
                        for(int pi = 0; pi < NI; ++pi)
                        {
                            if(cand[pi] == ~0u) { cost[pi] += x.steps; continue; }
                            have_i[pi]++;
                            bool occ;
                            cost[pi] += inst_first(x.q, cand[pi], occ, cprim[pi]);
                            if(occ != x.occ) ++wrong;
                            hit_i[pi] += (occ && x.occ) ? 1 : 0;
                        }
                        if(x.occ) { wave_last = x.oi; wave_last_p = x.op; pix[x.pixel] = x.oi; }
                    }
                    if(wave_last != ~0u) { group_last = wave_last; group_last_p = wave_last_p; }
                }
            }
            for(int pi = 0; pi < NI; ++pi)
                printf("  instance-first %-20s candidate for %5.1f%%, occluded via it or after %5.1f%% of occluded; steps %+.1f%% vs the walk\n",
                       in_names[pi], 100 * have_i[pi] / tot_q, 100 * hit_i[pi] / std::max(1.0, tot_occ), 100 * (cost[pi] - steps_all) / steps_all);
        }
        printf("  %llu wrong (block walk vs link walk, or an accepted candidate on an unoccluded ray); %llu of %llu tests "
               "failed the TLAS membership\n", (unsigned long long)wrong, (unsigned long long)test_fail_membership,
               (unsigned long long)tests);
        return wrong ? 1 : 0;
    }

    // ANYHIER: a second scene whose BLASes are rebuilt with another SAH
    // traversal cost (tools/Makefile walk_simh); its instances, meshes and
    // TLAS leaves must be the first scene's
    ptg_scene* sceneB = nullptr;
    ptg_scene_view vB{};
    Packed pkB;
    if(const char* hc = getenv("ANYHIER"))
    {
#ifdef PTG_MODEL_HOOKS
        g_model_blas_traversal_cost = float(atof(hc));
        const int e1 = ptg_scene_load(argv[1], &cfg, &sceneB);
        g_model_blas_traversal_cost = 2.0f;
        if(e1 || ptg_scene_setup_frame(sceneB, frame)) { fprintf(stderr, "ANYHIER scene: %s\n", ptg_last_error()); return 1; }
        ptg_scene_view_get(sceneB, &vB);
        size_t diff = vB.instance_count != v.instance_count ? 1 : 0;
        for(size_t i = 0; !diff && i < v.instance_count; ++i)
            diff += memcmp(&v.instances[i].m, &vB.instances[i].m, sizeof(ptg_mesh)) ||
                    memcmp(&v.instances[i].transform, &vB.instances[i].transform, 2 * sizeof(v.instances[i].transform));
        BlockCache cB;
        cB.set_scene(vB.nodes, vB.links, vB.static_node_count, vB.indices, vB.index_count, vB.pos, vB.albedo, vB.material,
                     vB.vertex_count);
        FramePack fB;
        if(cB.pack_frame(vB.subframes, vB.subframe_count, vB.instances, vB.instance_count, vB.nodes + vB.static_node_count,
                         vB.links + 8 * vB.static_node_count, vB.static_node_count, vB.node_count - vB.static_node_count, fB, err))
        { fprintf(stderr, "ANYHIER pack: %s\n", err.c_str()); return 1; }
        pkB.E = fB.new_blas;
        pkB.E.insert(pkB.E.end(), fB.tlas.begin(), fB.tlas.end());
        pkB.inst_root = fB.inst_root;
        pkB.tlas_root = fB.tlas_root;
        printf("ANYHIER cost %s: static nodes %zu (reference %zu); BLAS blocks %.1f MB (reference %.1f MB); instances differing %zu\n",
               hc, vB.static_node_count, v.static_node_count, fB.new_blas.size() * 128 / 1e6,
               (cache.blas.size() + fp.new_blas.size()) * 128 / 1e6, diff);
        if(diff) return 1;
#else
        fprintf(stderr, "ANYHIER needs the walk_simh build (tools/Makefile)\n");
        return 2;
#endif
    }

    // the query mix
    std::vector<Query> qs;
    const bool tiled = getenv("CACHESIM") != nullptr;   // paths in the device's queue order: 8 pixels x 8 samples per wave
    const uint32_t x0 = uint32_t(rnd() * (cfg.width / 2)), y0 = uint32_t(rnd() * (cfg.height / 2));
    for(uint32_t p = 0; p < paths; ++p)
    {
        uint32_t px = uint32_t(rnd() * cfg.width), py = uint32_t(rnd() * cfg.height);
        uint32_t sf = uint32_t(rnd() * v.subframe_count) % v.subframe_count;
        if(tiled)
        {   // wave g = p / 64: pixels 8 (g % 80) .. +7 of row y0 + g / 80; lane: pixel (p % 64) / 8, sample p % 8
            const uint32_t g = p / 64, lane = p % 64;
            px = (x0 + 8 * (g % 80) + lane / 8) % cfg.width;
            py = (y0 + g / 80) % cfg.height;
            sf = (g * 8 / 8) % v.subframe_count;
        }
        const ptg_camera& cam = v.subframes[sf].cam;
        float ux = (px + 0.5f) / cfg.width * 2.0f - 1.0f, uy = (py + 0.5f) / cfg.height * 2.0f - 1.0f;
        ux *= cam.aspect_ratio;
        uy = -uy;
        f3 d = normalize(v3(ux * cam.inv_focal_length, uy * cam.inv_focal_length, -1.0f));
        d = mul_m3v3(cam.orientation, d);
        f3 o = cam.position;
        uint32_t src = 0xFFFFu;   // the instance the ray leaves (camera: none)
        for(uint32_t bnc = 0; bnc <= 4; ++bnc)
        {
            Query q{o, d, bnc ? 1e-4f : 0.0f, 1e9f, sf, false, bnc, src};
            qs.push_back(q);
            Stats tmp;
            Res r = link_walk(v, q, tmp);
            if(r.inst == 0xFFFFFFFFu) break;
            o = o + d * r.t;
            f3 L = normalize(v.subframes[sf].light.direction);
            src = r.inst;
            qs.push_back(Query{o, L, 1e-4f, 1e9f, sf, true, bnc, src});
            {   // model of the surface pass's untraced shadow rays (path_tracer.h attenuation_steps):
                // the sun ray's atmosphere integral has a step below the ground (float arithmetic
                // as the device's, the jitter drawn here)
                static uint64_t n_sh = 0, n_blocked = 0;
                const float R = 6.3781e6f, H = 1.0e5f;
                const f3 oc = o - v3(0, -R, 0);
                const float b = dot(oc, L), cc = dot(oc, oc) - (R + H) * (R + H);
                float disc = b * b - cc;
                bool blocked = false;
                if(disc >= 0)
                {
                    disc = std::sqrt(disc);
                    float tmin = -b - disc, tmax = -b + disc;
                    tmin = float(std::max(double(tmin), 0.0));
                    tmax = std::min(tmax, 1e9f);
                    const float seg = (tmax - tmin) / 8.0f, jit = rnd();
                    for(int i = 0; i < 8 && !blocked; ++i)
                    {
                        const f3 pp = o + L * (seg * (jit + float(i))) - v3(0, -R, 0);
                        blocked = std::sqrt(dot(pp, pp)) - R < 0;
                    }
                }
                ++n_sh;
                n_blocked += blocked;
                if((n_sh & (n_sh - 1)) == 0 && n_sh >= 1024)
                    fprintf(stderr, "shadow rays whose sun ray is blocked by the ground: %.1f%% of %llu\n",
                            100.0 * double(n_blocked) / double(n_sh), (unsigned long long)n_sh);
            }
            f3 nd;
            do { nd = v3(rnd() * 2 - 1, rnd() * 2 - 1, rnd() * 2 - 1); } while(dot(nd, nd) > 1 || dot(nd, nd) < 1e-4f);
            static const bool axis_dirs = getenv("AXIS") != nullptr;   // bounces with zero / NaN direction components
            if(axis_dirs && rnd() < 0.02f)
            {   // a NaN direction (one, two or all three components), as a degenerate shading frame makes
                const float qn = std::numeric_limits<float>::quiet_NaN();
                f3 bad = nd;
                const int k = int(rnd() * 3) % 3, cnt = 1 + int(rnd() * 3) % 3;
                for(int c = 0; c < cnt; ++c) ((k + c) % 3 == 0 ? bad.x : (k + c) % 3 == 1 ? bad.y : bad.z) = qn;
                qs.push_back(Query{o, bad, 1e-4f, 1e9f, sf, false, bnc, src});
                qs.push_back(Query{o, bad, 1e-4f, 1e9f, sf, true, bnc, src});
            }
            if(axis_dirs && rnd() < 0.5f)
            {   // one or two components exactly zero (1/dir infinite: the walk's min/max form)
                const int k = int(rnd() * 3) % 3;
                (k == 0 ? nd.x : k == 1 ? nd.y : nd.z) = 0.0f;
                if(rnd() < 0.3f) (k == 0 ? nd.y : k == 1 ? nd.z : nd.x) = 0.0f;
                if(dot(nd, nd) < 1e-4f) nd = v3(0, 1, 0);
            }
            nd = normalize(nd);
            if(dot(nd, d) > 0) nd = -nd;
            d = nd;
        }
    }
    {
        size_t zero = 0;
        for(const Query& q: qs) zero += (q.d.x == 0.0f || q.d.y == 0.0f || q.d.z == 0.0f) ? 1 : 0;
        printf("queries with a zero direction component: %zu of %zu\n", zero, qs.size());
    }
    if(const char* cs = getenv("CACHESIM"))
    {   // Cache behaviour of the walk kernel's access stream on one slice of
        // an XCD: W lockstep waves (12 per CU) stepping round-robin, wave w
        // taking the queue's 64-entry groups w, w + W, ... of each round (the
        // kernel's static split), 2 node phases + 1 leaf phase per
        // iteration, refill at 24 idle lanes.  Each lane's 128 B lines go
        // through its CU's L1 (32 KB, 64-way LRU sets) and the slice's share of
        // L2 (4 MB per 32 CUs, 16-way).  CACHESIM="order": 0 queue order,
        // 1 each round's queue sorted by ray octant (stable).
        const int order = atoi(cs);
        const int W = 96, per_cu = 12;
        struct Cache {
            uint32_t sets, ways;
            std::vector<uint64_t> tag, age;
            uint64_t clock = 0, hits = 0, miss = 0;
            Cache(uint32_t lines, uint32_t w) : sets(lines / w), ways(w), tag(size_t(lines), ~0ull), age(size_t(lines), 0) {}
            bool access(uint64_t line)
            {
                const size_t s0 = size_t(line % sets) * ways;
                ++clock;
                size_t lru = s0;
                for(size_t k = s0; k < s0 + ways; ++k)
                {
                    if(tag[k] == line) { age[k] = clock; ++hits; return true; }
                    if(age[k] < age[lru]) lru = k;
                }
                tag[lru] = line; age[lru] = clock; ++miss;
                return false;
            }
        };
        for(int any = 0; any < 2; ++any)
        {
            std::vector<Cache> l1(W / per_cu, Cache(256, 64));
            Cache l2(uint32_t((4u << 20) / 128 * (W / per_cu) / 32), 16);
            double node_ph = 0, leaf_ph = 0, nq = 0;
            for(uint32_t rd = 0; rd <= 4; ++rd)
            {
                std::vector<const Query*> qq;
                for(const Query& q: qs)
                    if(q.any == bool(any) && q.round == rd) qq.push_back(&q);
                if(order == 1)
                    std::stable_sort(qq.begin(), qq.end(), [](const Query* a, const Query* b) { return octant(a->d) < octant(b->d); });
                else if(order == 4 || order == 5)
                {   // octant-sorted within each run of 256 (a shade block's append) or 2048 queue entries
                    const size_t run = order == 4 ? 256 : 2048;
                    for(size_t i = 0; i < qq.size(); i += run)
                        std::stable_sort(qq.begin() + i, qq.begin() + std::min(qq.size(), i + run),
                                         [](const Query* a, const Query* b) { return octant(a->d) < octant(b->d); });
                }
                else if(order == 7 || order == 8)
                {   // the device's key: 12-bit Morton hash of the origin's cell (CELL metres), ties by queue order;
                    // 8: the octant and a 9-bit hash
                    static const float cell = getenv("CELL") ? float(atof(getenv("CELL"))) : 2.0f;
                    auto key = [&](const Query* q) {
                        auto sp = [](int32_t c) {
                            uint32_t x = uint32_t(c) & 15u;
                            x = (x | (x << 4)) & 0x0C3u; x = (x | (x << 2)) & 0x249u;
                            return x;
                        };
                        const int32_t cx = int32_t(std::floor(q->o.x / cell)), cy = int32_t(std::floor(q->o.y / cell)),
                                      cz = int32_t(std::floor(q->o.z / cell));
                        const uint32_t m = sp(cx) | (sp(cy) << 1) | (sp(cz) << 2);
                        return order == 7 ? m : (octant(q->d) << 9) | (m & 511u);
                    };
                    std::stable_sort(qq.begin(), qq.end(), [&](const Query* a, const Query* b) { return key(a) < key(b); });
                }
                else if(order == 6)
                    std::stable_sort(qq.begin(), qq.end(), [](const Query* a, const Query* b) {
                        return (uint64_t(octant(a->d)) << 32 | a->src) < (uint64_t(octant(b->d)) << 32 | b->src); });
                else if(order >= 2 && !qq.empty())
                {   // Morton order of the ray origins (10 bits per axis over the round's origin bounds), octant first (2) or not (3)
                    f3 lo = qq[0]->o, hi = qq[0]->o;
                    for(const Query* q: qq)
                    {
                        lo = v3(std::min(lo.x, q->o.x), std::min(lo.y, q->o.y), std::min(lo.z, q->o.z));
                        hi = v3(std::max(hi.x, q->o.x), std::max(hi.y, q->o.y), std::max(hi.z, q->o.z));
                    }
                    auto spread = [](uint64_t x) {
                        x &= 0x3FF;
                        x = (x | (x << 16)) & 0x030000FF; x = (x | (x << 8)) & 0x0300F00F;
                        x = (x | (x << 4)) & 0x030C30C3; x = (x | (x << 2)) & 0x09249249;
                        return x;
                    };
                    auto key = [&](const Query* q) {
                        auto qz = [](float a, float l, float h) { return uint64_t(std::min(1023.0f, (a - l) / std::max(h - l, 1e-20f) * 1024.0f)); };
                        const uint64_t m = spread(qz(q->o.x, lo.x, hi.x)) | (spread(qz(q->o.y, lo.y, hi.y)) << 1) | (spread(qz(q->o.z, lo.z, hi.z)) << 2);
                        return order == 2 ? (uint64_t(octant(q->d)) << 30) | m : m;
                    };
                    std::stable_sort(qq.begin(), qq.end(), [&](const Query* a, const Query* b) { return key(a) < key(b); });
                }
                nq += double(qq.size());
                const size_t groups = (qq.size() + 63) / 64;
                struct WaveSt { std::vector<std::unique_ptr<SimWalker>> lane; std::vector<Stats> st; size_t g, used; };
                std::vector<WaveSt> ws(W);
                for(int w = 0; w < W; ++w) { ws[w].lane.resize(64); ws[w].st.resize(64); ws[w].g = size_t(w); ws[w].used = 0; }
                auto next_query = [&](WaveSt& x) -> const Query* {
                    while(x.g < groups)
                    {
                        const size_t i = x.g * 64 + x.used;
                        if(x.used < 64 && i < qq.size()) { ++x.used; return qq[i]; }
                        x.g += W; x.used = 0;
                    }
                    return nullptr;
                };
                std::vector<uint64_t> lines;
                g_lines = &lines;
                for(bool live = true; live;)
                {
                    live = false;
                    for(int w = 0; w < W; ++w)
                    {
                        WaveSt& x = ws[w];
                        Cache& c1 = l1[w / per_cu];
                        int idle = 0;
                        for(auto& l: x.lane) idle += l ? 0 : 1;
                        if(idle >= 24 || idle == 64)
                            for(int k = 0; k < 64; ++k)
                                if(!x.lane[k])
                                    if(const Query* q = next_query(x)) x.lane[k].reset(new SimWalker(v, pk, *q, x.st[k], S, g_spec));
                        bool any_live = false;
                        for(auto& l: x.lane) any_live = any_live || bool(l);
                        if(!any_live) continue;
                        live = true;
                        auto feed = [&](double& ph) {
                            if(lines.empty()) return;
                            ph += 1;
                            for(uint64_t ln: lines)
                                if(!c1.access(ln)) l2.access(ln);
                            lines.clear();
                        };
                        for(int u = 0; u < 2; ++u)
                        {
                            for(auto& l: x.lane)
                            {
                                if(!l || l->at_leaf()) continue;
                                bool ld;
                                if(l->dev_node_phase(1, ld)) l.reset();
                            }
                            feed(node_ph);
                        }
                        for(auto& l: x.lane)
                            if(l && l->wants_leaf() && l->leaf_step()) l.reset();
                        feed(leaf_ph);
                    }
                }
                g_lines = nullptr;
            }
            uint64_t h1 = 0, m1 = 0;
            for(auto& c: l1) { h1 += c.hits; m1 += c.miss; }
            printf("cachesim %s order=%d: %.0f queries, L1 hit %.1f%%, L2 hit %.1f%% of L1 misses, L2 misses %.2f per query, L1 misses %.2f per query\n",
                   any ? "any" : "closest", order, nq, 100.0 * h1 / double(h1 + m1), 100.0 * l2.hits / double(l2.hits + l2.miss),
                   l2.miss / nq, m1 / nq);
        }
        return 0;
    }
    if(const char* ls = getenv("LOCKSTEP"))
    {   // the wavefront walk kernel's lockstep schedule over the query mix,
        // per walk kind, in waves of 64 lanes with the kernel's refill rule:
        // vector-memory instructions (7 per node phase that reads a block, 4
        // per leaf phase that reads a record, 3 per refill) and the lanes each
        // serves.  LOCKSTEP="U K T": U node phases per leaf phase, K pops per
        // node phase, leaf phase only when >= T lanes want one (or no lane
        // can take a node step).
        const double kRows = (28.0 * kBlockWidth + 15) / 16;   // 16-byte rows a block step reads (7 at width 4)
        int U = 2, K = 1, T = 1, R = 24, E = 1;   // E: BLAS entries only in every E-th leaf phase
        sscanf(ls, "%d %d %d %d %d", &U, &K, &T, &R, &E);
        for(int any = 0; any < 2; ++any)
        {
            std::vector<const Query*> mine;
            for(const Query& q: qs)
                if(q.any == bool(any)) mine.push_back(&q);
            double ni = 0, nl = 0, li = 0, ll = 0, ri = 0, rl = 0, phases = 0, iters = 0, waves = 0, act = 0, leaf_ph = 0, leaf_ph_enter = 0, rph = 0;
            double leaf_ph_tri = 0;
            const size_t per_wave = 4096;   // queries one wave works through (its range)
            uint64_t lmism = 0;
            double why[5] = {};   // node-phase lanes not reading a block: instance leaf, triangle leaf, parked & waiting, popped nothing steppable, empty
            auto check = [&](const SimWalker& w) {   // every finished walk against the reference's link walk
                Stats tmp;
                if(!(link_walk(v, w.q, tmp) == w.best)) ++lmism;
            };
            for(size_t w0 = 0; w0 < mine.size(); w0 += per_wave)
            {
                const size_t end = std::min(mine.size(), w0 + per_wave);
                size_t next = w0;
                std::vector<Stats> lst(64);
                std::vector<std::unique_ptr<SimWalker>> lane(64);
                waves++;
                for(;;)
                {
                    int idle = 0;
                    for(auto& l: lane) idle += l ? 0 : 1;
                    if(next < end && (idle >= R || idle == 64))
                    {
                        int took = 0;
                        for(int k = 0; k < 64 && next < end; ++k)
                            if(!lane[k]) { lane[k].reset(new SimWalker(v, pk, *mine[next++], lst[k], S, g_spec)); ++took; }
                        ri += 3; rl += 3 * took; rph++;
                    }
                    int live = 0;
                    for(auto& l: lane) live += l ? 1 : 0;
                    if(!live) break;
                    iters++;
                    act += live;
                    for(int u = 0; u < U; ++u)
                    {
                        int loads = 0;
                        for(auto& l: lane)
                        {
                            if(l && l->at_leaf()) { why[l->axis < 0 ? 0 : 1]++; continue; }
                            if(!l) { why[4]++; continue; }
                            bool ld;
                            if(l->dev_node_phase(K, ld)) { check(*l); l.reset(); }
                            loads += ld ? 1 : 0;
                            if(l && !ld) why[l->pend != kBePop && l->cur == kBePop ? 2 : 3]++;
                        }
                        if(loads) { ni += kRows; nl += kRows * loads; phases++; }
                    }
                    int want = 0, can_node = 0;
                    for(auto& l: lane)
                        if(l) { want += l->wants_leaf() ? 1 : 0; can_node += l->at_leaf() ? 0 : 1; }
                    const bool entry_phase = E <= 1 || (uint64_t(iters) % uint64_t(E)) == 0;
                    if(want && (want >= T || can_node == 0 || want == live))
                    {
                        int loads = 0, enters = 0, tris = 0;
                        for(auto& l: lane)
                        {
                            if(!l || !l->wants_leaf()) continue;
                            if(!entry_phase && l->axis < 0 && l->pend == kBePop) continue;   // its BLAS entry waits
                            const double t0 = l->st.tri;
                            const double before = l->st.tri + l->st.enters, e0 = l->st.enters;
                            const int r = l->leaf_step();
                            loads += (l->st.tri + l->st.enters > before) ? 1 : 0;
                            enters += (l->st.enters > e0) ? 1 : 0;
                            tris += (l->st.tri > t0) ? 1 : 0;
                            if(r) { check(*l); l.reset(); }
                        }
                        if(loads) { li += 4; ll += 4 * loads; phases++; leaf_ph++; leaf_ph_enter += enters ? 1 : 0; leaf_ph_tri += tris ? 1 : 0; }
                    }
                }
            }
            const double nq = double(mine.size());
            printf("lockstep %s U=%d K=%d T=%d: per query %.2f VMEM (node %.2f, leaf %.2f, refill %.2f), %.1f phases with loads per wave-query64, lanes/instr node %.1f leaf %.1f, active %.1f\n",
                   any ? "any" : "closest", U, K, T, (ni + li + ri) * 64 / nq, ni * 64 / nq, li * 64 / nq, ri * 64 / nq,
                   phases * 64 / nq, nl / std::max(ni, 1.0), ll / std::max(li, 1.0), act / std::max(iters, 1.0));
            const double tot_ph = ni / kRows;
            printf("  per node phase, lanes not reading: at instance %.1f, at triangle %.1f, parked+stalled %.1f, popped none %.1f, empty %.1f\n",
                   why[0] / tot_ph, why[1] / tot_ph, why[2] / tot_ph, why[3] / tot_ph, why[4] / tot_ph);
            printf("  refill phases %.2f per wave-query64 (R=%d)\n", rph * 64 / nq, R);
            printf("  leaf phases with a BLAS entry: %.1f%%; %llu mismatches vs the link walk\n",
                   100.0 * leaf_ph_enter / std::max(leaf_ph, 1.0), (unsigned long long)lmism);
            printf("  per 64 queries: %.1f iterations, %.1f node phases with loads, %.1f leaf phases with an entry, %.1f with a triangle (E=%d)\n",
                   iters * 64 / nq, ni / kRows * 64 / nq, leaf_ph_enter * 64 / nq, leaf_ph_tri * 64 / nq, E);
        }
        return 0;
    }
    Stats sl[2], sb[2], sh;
    uint64_t mism = 0, mismh = 0;
    for(const Query& q: qs)
    {
        Res a = link_walk(v, q, sl[q.any]);
        Res b = block_walk(v, pk, q, sb[q.any], S);
        if(sceneB && q.any)
        {
            const Res c = block_walk(vB, pkB, q, sh, S);
            if(!(a == c) && mismh++ < 5)
                fprintf(stderr, "ANYHIER mismatch: link occ=%d | rebuilt occ=%d\n", a.occluded, c.occluded);
        }
        if(getenv("CLOSEBOUND") && !q.any && b.inst != 0xFFFFFFFFu)
        {   // model: the closest-hit walk started with tmax = next float above the
            // final hit's t (a perfect neighbour candidate); same result, fewer steps?
            static Stats cb, base;
            static uint64_t nq = 0, wrong = 0;
            Query q2 = q;
            q2.tmax = std::nextafter(b.t, INFINITY);
            Stats tmp;
            const Res c = block_walk(v, pk, q2, cb, S);
            block_walk(v, pk, q, base, S);
            if(!(c == b) && wrong++ < 4)
                fprintf(stderr, "  differ: t %a inst %u prim %u u %a | bounded t %a inst %u prim %u u %a\n", b.t, b.inst, b.prim, b.u,
                        c.t, c.inst, c.prim, c.u);
            if(++nq % 20000 == 0 || nq == 1)
                fprintf(stderr, "CLOSEBOUND: %llu hit queries, %llu differ; block steps %.2f -> %.2f, box tests %.1f -> %.1f\n",
                        (unsigned long long)nq, (unsigned long long)wrong, base.block_steps / base.queries, cb.block_steps / cb.queries,
                        base.visits / base.queries, cb.visits / cb.queries);
        }
        if(!(a == b))
        {
            if(mism < 5)
                fprintf(stderr, "mismatch: any=%d link t=%a inst=%u prim=%u occ=%d | block t=%a inst=%u prim=%u occ=%d\n", q.any,
                        a.t, a.inst, a.prim, a.occluded, b.t, b.inst, b.prim, b.occluded);
            ++mism;
        }
    }
    printf("%zu queries, %llu mismatches\n", qs.size(), (unsigned long long)mism);
    printf("most block-walk steps of one query: %.0f\n", g_max_query_steps);
    for(int k = 0; k < 2; ++k)
    {
        const Stats& a = sl[k];
        const Stats& b = sb[k];
        printf("%s: %.0f queries\n", k ? "shadow (any)" : "closest", a.queries);
        printf("  link : visits %.1f  steps %.1f  dep-loads %.1f  tri %.2f  enters %.2f  bytes %.0f\n", a.visits / a.queries,
               a.steps / a.queries, a.dep_loads / a.queries, a.tri / a.queries, a.enters / a.queries, a.bytes / a.queries);
        printf("  block: boxes %.1f  steps %.1f (block %.1f, leaf %.1f)  tri %.2f  enters %.2f  pushes %.1f  spills(S=%u) %.3f  iters %.1f  bytes %.0f\n",
               b.visits / b.queries, b.steps / b.queries, b.block_steps / b.queries, b.leaf_steps / b.queries, b.tri / b.queries,
               b.enters / b.queries, b.pushes / b.queries, S, b.spills / b.queries, b.iters / b.queries, b.bytes / b.queries);
        uint64_t acc = 0;
        printf("  max stack depth CDF:");
        for(auto& kv: b.depth_hist)
        {
            acc += kv.second;
            printf(" %u:%.4f", kv.first, acc / b.queries);
        }
        printf("\n");
    }
    if(sceneB)
    {
        const Stats& b = sb[1];
        printf("ANYHIER any-hit over the rebuilt BLASes: %llu mismatches vs the link walk\n", (unsigned long long)mismh);
        printf("  reference tree: boxes %.1f  steps %.2f (block %.2f, leaf %.2f)  tri %.2f  enters %.2f  iters %.1f  bytes %.0f\n",
               b.visits / b.queries, b.steps / b.queries, b.block_steps / b.queries, b.leaf_steps / b.queries, b.tri / b.queries,
               b.enters / b.queries, b.iters / b.queries, b.bytes / b.queries);
        printf("  rebuilt tree  : boxes %.1f  steps %.2f (block %.2f, leaf %.2f)  tri %.2f  enters %.2f  iters %.1f  bytes %.0f\n",
               sh.visits / sh.queries, sh.steps / sh.queries, sh.block_steps / sh.queries, sh.leaf_steps / sh.queries,
               sh.tri / sh.queries, sh.enters / sh.queries, sh.iters / sh.queries, sh.bytes / sh.queries);
        ptg_scene_destroy(sceneB);
    }
    ptg_scene_destroy(scene);
    return (mism || mismh) ? 1 : 0;
}
