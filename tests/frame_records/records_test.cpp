// CPU test of the per-frame records BlockCache::pack_frame builds
// (host/block_bvh.cpp): InstTrav, InstShade, InstBox and the mesh jobs.
//
//   records_test                 synthetic frames built with the project's own
//                                builder (build_blas / build_tlas): every InstBox
//                                class, the record bytes, the leaf-box gate and its
//                                memo, transactionality, the mesh jobs
//   records_test real <assets>   frames 0, 450 and 1400 of the real scene (frame 0
//                                committed first): SHA-256 of each record array
//                                and the instances per class, for
//                                tests/golden/frame_records.json
#include "ptg.h"
#include "host/block_bvh.h"
#include "host/scene_internal.h"
#include "sha256.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace ptg;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if(!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while(0)

ptg_float3 p3(float x, float y, float z) { ptg_float3 r{}; r.x = x; r.y = y; r.z = z; return r; }
ptg_float4 p4(float x, float y, float z, float w) { ptg_float4 r{}; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// Two meshes of two triangles each (a unit quad in z = 0; the second one
// stretched), each with its own BLAS: A at index_offset 0, B at 6.
struct Scene {
    MeshBuffers mb;
    BvhBuffers bvh;   // [BLAS A][BLAS B], then the TLASes of the frame being built
    ptg_mesh mesh[2];
    ptg_bvh blas[2];
    size_t static_nodes = 0;
    Scene()
    {
        const float sx[2] = {1.0f, 2.0f};
        for(uint32_t m = 0; m < 2; ++m)
        {
            mesh[m] = ptg_mesh{4, 2, uint32_t(mb.indices.size()), uint32_t(mb.pos.size())};
            for(uint32_t i: {0u, 1u, 2u, 0u, 2u, 3u}) mb.indices.push_back(i);
            for(ptg_float3 p: {p3(0, 0, 0), p3(sx[m], 0, 0), p3(sx[m], 1, 0), p3(0, 1, 0)})
            {
                mb.pos.push_back(p);
                mb.normal.push_back(p3(0, 0, 1));
                mb.albedo.push_back(p4(0.5f, 0.5f, 0.5f, 1));
                mb.material.push_back(p4(0, 0, 0, 0));
            }
            blas[m] = build_blas(mesh[m], mb, bvh);
        }
        static_nodes = bvh.nodes.size();
    }
    void set(BlockCache& c) const
    {
        c.set_scene(bvh.nodes.data(), bvh.links.data(), static_nodes, mb.indices.data(), mb.indices.size(), mb.pos.data(),
                    mb.albedo.data(), mb.material.data(), mb.pos.size());
    }
    // an instance of mesh m translated by (tx, ty, tz); inv_transform holds
    // recognisable numbers (pack_frame copies it, nothing inverts it)
    ptg_tlas_instance instance(uint32_t m, float tx, float ty, float tz, float tag) const
    {
        ptg_tlas_instance in{};
        in.blas = blas[m];
        in.m = mesh[m];
        in.transform.r[0] = p4(1, 0, 0, 0);
        in.transform.r[1] = p4(0, 1, 0, 0);
        in.transform.r[2] = p4(0, 0, 1, 0);
        in.transform.r[3] = p4(tx, ty, tz, 1);   // y_k = sum_j r[j][k] * x_j (math.hh:224-228)
        for(int k = 0; k < 4; ++k) in.inv_transform.r[k] = p4(tag + k + 0.25f, tag + k + 0.5f, tag + k + 0.75f, -tag);
        return in;
    }
};

// A frame: the instances and, per subframe, the TLAS over the instances it names.
struct Frame {
    Scene& sc;
    std::vector<ptg_tlas_instance> inst;
    std::vector<ptg_subframe> sub;
    explicit Frame(Scene& s): sc(s)
    {
        sc.bvh.nodes.resize(sc.static_nodes);
        sc.bvh.links.resize(sc.static_nodes * 8);
    }
    // `moved`: instances this subframe's TLAS sees translated by +4 in x
    void subframe(const std::vector<uint32_t>& ids, const std::vector<uint32_t>& moved = {})
    {
        std::vector<ptg_tlas_instance> local = inst;
        for(uint32_t i: moved) local[i].transform.r[3].x += 4.0f;
        std::vector<const ptg_tlas_instance*> ptr;
        for(uint32_t i: ids) ptr.push_back(&local[i]);
        ptg_subframe s{};
        s.tlas = build_tlas(ids.size(), ptr.data(), ids.data(), sc.bvh, sc.bvh);
        sub.push_back(s);
    }
    int pack(const BlockCache& c, FramePack& fp, std::string& err) const
    {
        return c.pack_frame(sub.data(), sub.size(), inst.data(), inst.size(), sc.bvh.nodes.data() + sc.static_nodes,
                            sc.bvh.links.data() + 8 * sc.static_nodes, sc.static_nodes, sc.bvh.nodes.size() - sc.static_nodes,
                            fp, err);
    }
    // the TLAS leaf node of subframe sf that names instance i (order 7's links)
    const ptg_bvh_node* leaf(size_t sf, uint32_t i) const
    {
        const ptg_bvh t = sub[sf].tlas;
        for(uint32_t n = 0; n < t.node_count; ++n)
            if(sc.bvh.links[size_t(t.node_offset) * 8 + size_t(7) * t.node_count + n].accept == (0x80000000u | i))
                return &sc.bvh.nodes[t.node_offset + n];
        return nullptr;
    }
    // makes every leaf of subframe sf's TLAS that names `from` name `to`, in all eight link orders
    void rename_leaf(size_t sf, uint32_t from, uint32_t to)
    {
        const ptg_bvh t = sub[sf].tlas;
        for(size_t k = 0; k < size_t(8) * t.node_count; ++k)
        {
            ptg_bvh_link& l = sc.bvh.links[size_t(t.node_offset) * 8 + k];
            if(l.accept == (0x80000000u | from)) l.accept = 0x80000000u | to;
        }
    }
};

bool box_is(const InstBox& b, uint32_t sub, const float (&lo)[3], const float (&hi)[3], uint32_t tris)
{
    const InstBox want{{lo[0], lo[1], lo[2]}, sub, {hi[0], hi[1], hi[2]}, tris};
    return memcmp(&b, &want, sizeof(InstBox)) == 0;
}
bool box_is_node(const InstBox& b, const ptg_bvh_node* n)
{
    return n && memcmp(b.lo, &n->min_x, 12) == 0 && memcmp(b.hi, &n->max_x, 12) == 0;
}
// never a candidate: the box bytes are whatever the first leaf left there
bool never(const InstBox& b, uint32_t tris) { return b.sub == kInstNoCandidate && b.tri_count == tris; }

template<class T> bool same_bytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
bool same_pack(const FramePack& a, const FramePack& b)
{
    if(a.new_records.size() != b.new_records.size()) return false;
    for(const auto& kv: a.new_records)
    {
        auto o = b.new_records.find(kv.first);
        if(o == b.new_records.end() || memcmp(&o->second, &kv.second, sizeof(BlasRecord)) != 0) return false;
    }
    return a.blas_base == b.blas_base && a.tlas_base == b.tlas_base && same_bytes(a.new_blas, b.new_blas) &&
           same_bytes(a.tlas, b.tlas) && same_bytes(a.tlas_root, b.tlas_root) && same_bytes(a.inst_root, b.inst_root) &&
           a.blas_stack == b.blas_stack && a.tlas_stack == b.tlas_stack && same_bytes(a.inst_trav, b.inst_trav) &&
           same_bytes(a.inst_shade, b.inst_shade) && same_bytes(a.inst_box, b.inst_box) &&
           same_bytes(a.mesh_jobs, b.mesh_jobs) && a.new_mesh == b.new_mesh;
}

// (a) every class of instance and the bytes of its three records
void test_classes()
{
    Scene sc;
    BlockCache c;
    sc.set(c);
    FramePack fp;
    std::string err;
    {   // two subframes: static, dynamic (subframe 1), moving, dynamic (subframe 0)
        Frame f(sc);
        f.inst = {sc.instance(1, 8, 0, 0, 100), sc.instance(0, 0, 8, 0, 200), sc.instance(0, 0, 0, 8, 300),
                  sc.instance(1, 16, 16, 0, 400)};
        f.subframe({0, 2, 3});
        f.subframe({0, 1, 2}, {2});
        CHECK(f.pack(c, fp, err) == PTG_OK);
        CHECK(fp.inst_box.size() == 4 && fp.inst_trav.size() == 4 && fp.inst_shade.size() == 4);
        // mesh B's quad is 2 x 1, mesh A's 1 x 1, both in z = 0: the leaf box is the quad's translated
        CHECK(box_is(fp.inst_box[0], kInstAllSubframes, {8, 0, 0}, {10, 1, 0}, 2));
        CHECK(box_is_node(fp.inst_box[0], f.leaf(0, 0)) && box_is_node(fp.inst_box[0], f.leaf(1, 0)));
        CHECK(box_is(fp.inst_box[1], 1, {0, 8, 0}, {1, 9, 0}, 2));
        CHECK(box_is_node(fp.inst_box[1], f.leaf(1, 1)) && !f.leaf(0, 1));
        CHECK(never(fp.inst_box[2], 2));
        CHECK(f.leaf(0, 2) && f.leaf(1, 2) && memcmp(f.leaf(0, 2), f.leaf(1, 2), sizeof(ptg_bvh_node)) != 0);
        CHECK(box_is(fp.inst_box[3], 0, {16, 16, 0}, {18, 17, 0}, 2));
        CHECK(box_is_node(fp.inst_box[3], f.leaf(0, 3)));

        // InstTrav / InstShade, written out by hand.  A fresh cache packs the
        // BLASes in order of first appearance, one block each (two leaves):
        // B's root is block 0, A's block 1; the triangle bases are
        // index_offset / 3 = 0 (A) and 2 (B).
        CHECK(fp.new_blas.size() == 2 * kBlockCopies && fp.blas_base == 0 && fp.tlas_base == 2);
        const uint32_t root[4] = {0, 1, 1, 0}, tri_base[4] = {2, 0, 0, 2};
        const float tag[4] = {100, 200, 300, 400};
        for(int i = 0; i < 4; ++i)
        {
            uint32_t trav[16], shade[16];
            for(uint32_t k = 0; k < 4; ++k)
            {
                trav[4 * k + 0] = bits(tag[i] + float(k) + 0.25f);
                trav[4 * k + 1] = bits(tag[i] + float(k) + 0.5f);
                trav[4 * k + 2] = bits(tag[i] + float(k) + 0.75f);
            }
            trav[3] = root[i]; trav[7] = tri_base[i]; trav[11] = 0; trav[15] = 0;
            const float rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            for(int k = 0; k < 9; ++k) shade[k] = bits(rot[k]);
            shade[9] = tri_base[i] * 3;          // index_offset
            shade[10] = tri_base[i] ? 4u : 0u;   // base_vertex_offset
            for(int k = 11; k < 16; ++k) shade[k] = 0;
            CHECK(memcmp(&fp.inst_trav[i], trav, 64) == 0);
            CHECK(memcmp(&fp.inst_shade[i], shade, 64) == 0);
        }
        // a rotated transform: InstShade takes rows 0..2 of `transform`, xyz each
        Frame g(sc);
        g.inst = {sc.instance(0, 1, 2, 3, 0), sc.instance(0, 4, 5, 6, 0)};
        g.inst[0].transform.r[0] = p4(0, 1, 0, 0);
        g.inst[0].transform.r[1] = p4(-1, 0, 0, 0);
        g.subframe({0, 1});
        CHECK(g.pack(c, fp, err) == PTG_OK);
        const float rot[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
        CHECK(memcmp(fp.inst_shade[0].rot, rot, 36) == 0);
        CHECK(box_is(fp.inst_box[0], 0, {0, 2, 3}, {1, 3, 3}, 2));   // one subframe: a leaf of exactly that one
    }
    {   // three subframes: static, dynamic (subframe 1), partial (0 and 1, not 2), moving (differs in 2)
        Frame f(sc);
        f.inst = {sc.instance(0, 8, 0, 0, 1), sc.instance(0, 0, 8, 0, 2), sc.instance(1, 0, 0, 8, 3), sc.instance(1, 16, 16, 0, 4)};
        f.subframe({0, 2, 3});
        f.subframe({0, 1, 2, 3});
        f.subframe({0, 3}, {3});
        CHECK(f.pack(c, fp, err) == PTG_OK);
        CHECK(box_is(fp.inst_box[0], kInstAllSubframes, {8, 0, 0}, {9, 1, 0}, 2));
        CHECK(box_is_node(fp.inst_box[0], f.leaf(0, 0)) && box_is_node(fp.inst_box[0], f.leaf(2, 0)));
        CHECK(box_is(fp.inst_box[1], 1, {0, 8, 0}, {1, 9, 0}, 2));
        CHECK(never(fp.inst_box[2], 2));
        CHECK(never(fp.inst_box[3], 2));
    }
}

// (b) one TLAS naming an instance twice: never a candidate, whichever subframe does it
void test_named_twice()
{
    Scene sc;
    BlockCache c;
    sc.set(c);
    FramePack fp;
    std::string err;
    for(size_t bad = 0; bad < 2; ++bad)
    {
        Frame f(sc);
        f.inst = {sc.instance(0, 8, 0, 0, 1), sc.instance(0, 0, 8, 0, 2), sc.instance(1, 0, 0, 8, 3)};
        f.subframe({0, 1, 2});
        f.subframe({0, 1, 2});
        f.rename_leaf(bad, 2, 1);   // subframe `bad` now names instance 1 twice and instance 2 not at all
        CHECK(f.pack(c, fp, err) == PTG_OK);
        CHECK(box_is(fp.inst_box[0], kInstAllSubframes, {8, 0, 0}, {9, 1, 0}, 2));
        CHECK(never(fp.inst_box[1], 2));
        CHECK(box_is(fp.inst_box[2], uint32_t(1 - bad), {0, 0, 8}, {2, 1, 8}, 2));
    }
    // the two leaves have the same box, and the instance is named as many
    // times as there are subframes: only the count of distinct subframes tells
    Frame f(sc);
    f.inst = {sc.instance(0, 8, 0, 0, 1), sc.instance(0, 0, 8, 0, 2), sc.instance(0, 0, 8, 0, 3), sc.instance(1, 0, 0, 8, 4)};
    f.subframe({0, 1, 2, 3});
    f.subframe({0, 1, 3});
    f.subframe({0, 3});
    CHECK(memcmp(f.leaf(0, 1), f.leaf(0, 2), sizeof(ptg_bvh_node)) == 0);
    f.rename_leaf(0, 2, 1);
    CHECK(f.pack(c, fp, err) == PTG_OK);
    CHECK(box_is(fp.inst_box[0], kInstAllSubframes, {8, 0, 0}, {9, 1, 0}, 2));
    CHECK(never(fp.inst_box[1], 2));
    CHECK(never(fp.inst_box[2], 2));   // named by no TLAS
    CHECK(box_is(fp.inst_box[3], kInstAllSubframes, {0, 0, 8}, {2, 1, 8}, 2));
}

// (c) the leaf-box gate: a BLAS with one leaf box off by one ulp offers no
// candidate triangles; the answer is memoised per (BLAS, mesh)
void test_leaf_box_gate()
{
    Scene sc;
    // a leaf of BLAS A, its box shrunk by one ulp (still inside its parent's)
    uint32_t leaf = 0;
    while(leaf < sc.blas[0].node_count && !(sc.bvh.links[leaf].accept & 0x80000000u)) ++leaf;
    CHECK(leaf > 0 && leaf < sc.blas[0].node_count);
    const ptg_bvh_node good = sc.bvh.nodes[leaf];
    sc.bvh.nodes[leaf].min_y = std::nextafter(good.min_y, 1.0f);
    BlockCache c;
    sc.set(c);
    Frame f(sc);
    f.inst = {sc.instance(0, 8, 0, 0, 1), sc.instance(1, 0, 8, 0, 2), sc.instance(0, 0, 0, 8, 3), sc.instance(1, 16, 16, 0, 4)};
    f.subframe({0, 1, 2, 3});
    f.subframe({0, 1, 2});
    FramePack fp;
    std::string err;
    auto tris = [&]() {
        CHECK(f.pack(c, fp, err) == PTG_OK);
        return std::vector<uint32_t>{fp.inst_box[0].tri_count, fp.inst_box[1].tri_count, fp.inst_box[2].tri_count,
                                     fp.inst_box[3].tri_count};
    };
    CHECK((tris() == std::vector<uint32_t>{0, 2, 0, 2}));
    CHECK(fp.inst_box[0].sub == kInstAllSubframes && fp.inst_box[3].sub == 0);   // the class does not depend on the gate
    CHECK(c.leaf_bounds_ok.size() == 2);
    // the memo answers the next frame: with the cache's copy of the box put
    // right behind its back the answer stays, and changes once the memo is dropped
    c.nodes[leaf] = good;
    CHECK((tris() == std::vector<uint32_t>{0, 2, 0, 2}));
    c.leaf_bounds_ok.clear();
    CHECK((tris() == std::vector<uint32_t>{2, 2, 2, 2}));
    // set_scene drops the memo with the scene
    sc.bvh.nodes[leaf].min_y = std::nextafter(good.min_y, 1.0f);
    sc.set(c);
    CHECK(c.leaf_bounds_ok.empty());
    CHECK((tris() == std::vector<uint32_t>{0, 2, 0, 2}));
}

// (d) a frame that fails leaves the cache as it was
void test_failed_frame()
{
    Scene sc;
    BlockCache c, fresh;
    sc.set(c);
    sc.set(fresh);
    FramePack fp, want;
    std::string err;
    Frame f(sc);
    f.inst = {sc.instance(0, 8, 0, 0, 1), sc.instance(1, 0, 8, 0, 2), sc.instance(1, 0, 0, 8, 3)};
    f.subframe({0, 1, 2});
    f.subframe({0, 1});
    std::vector<ptg_tlas_instance> good = f.inst;
    f.inst[2].m.triangle_count = 3;   // index_offset 6 + 9 indices > the 12 uploaded
    CHECK(f.pack(c, fp, err) == PTG_E_RANGE);
    CHECK(err == "instance 2: mesh outside the uploaded buffers");
    CHECK(c.blas.empty() && c.records.empty() && c.blas_stack == 0 && c.packed_mesh.empty());
    f.inst = good;
    CHECK(f.pack(c, fp, err) == PTG_OK);
    CHECK(f.pack(fresh, want, err) == PTG_OK);
    CHECK(same_pack(fp, want));
    CHECK(fp.mesh_jobs.size() == 2 && fp.new_blas.size() == 2 * kBlockCopies);
    // and an uncommitted good frame leaves it alone too
    CHECK(c.blas.empty() && c.records.empty() && c.blas_stack == 0 && c.packed_mesh.empty());
}

// (e) one mesh job per distinct index_offset no committed frame packed, by first appearance
void test_mesh_jobs()
{
    Scene sc;
    BlockCache c;
    sc.set(c);
    FramePack fp;
    std::string err;
    Frame f(sc);
    f.inst = {sc.instance(1, 8, 0, 0, 1), sc.instance(0, 0, 8, 0, 2), sc.instance(1, 0, 0, 8, 3), sc.instance(0, 16, 16, 0, 4)};
    f.subframe({0, 1, 2, 3});
    const MeshJob b_then_a[2] = {{6, 2, 4, 0}, {0, 2, 0, 0}};
    CHECK(f.pack(c, fp, err) == PTG_OK);
    CHECK(fp.mesh_jobs.size() == 2 && memcmp(fp.mesh_jobs.data(), b_then_a, sizeof(b_then_a)) == 0);
    CHECK((fp.new_mesh == std::unordered_set<uint32_t>{0, 6}));
    CHECK(f.pack(c, fp, err) == PTG_OK);   // not committed: the jobs are still due
    CHECK(fp.mesh_jobs.size() == 2 && memcmp(fp.mesh_jobs.data(), b_then_a, sizeof(b_then_a)) == 0);
    c.commit(fp);
    CHECK((c.packed_mesh == std::unordered_set<uint32_t>{0, 6}) && c.blas.size() == 2 * kBlockCopies && c.records.size() == 2);
    CHECK(f.pack(c, fp, err) == PTG_OK);
    CHECK(fp.mesh_jobs.empty() && fp.new_mesh.empty() && fp.new_blas.empty() && fp.blas_base == 2);
    CHECK(fp.inst_root == (std::vector<uint32_t>{0, 1, 0, 1}));
    sc.set(c);                             // a new scene: nothing of the old one is on the device
    CHECK(c.packed_mesh.empty() && c.blas.empty());
    CHECK(f.pack(c, fp, err) == PTG_OK);
    CHECK(fp.mesh_jobs.size() == 2 && memcmp(fp.mesh_jobs.data(), b_then_a, sizeof(b_then_a)) == 0);
    // a committed frame that names mesh A alone leaves B's job to the next one
    sc.set(c);
    Frame g(sc);
    g.inst = {sc.instance(0, 8, 0, 0, 1), sc.instance(0, 0, 8, 0, 2)};
    g.subframe({0, 1});
    CHECK(g.pack(c, fp, err) == PTG_OK);
    CHECK(fp.mesh_jobs.size() == 1 && memcmp(fp.mesh_jobs.data(), &b_then_a[1], sizeof(MeshJob)) == 0);
    c.commit(fp);
    Frame h(sc);
    h.inst = f.inst;
    h.subframe({0, 1, 2, 3});
    CHECK(h.pack(c, fp, err) == PTG_OK);
    CHECK(fp.mesh_jobs.size() == 1 && memcmp(fp.mesh_jobs.data(), &b_then_a[0], sizeof(MeshJob)) == 0);
    CHECK(fp.blas_base == 1 && fp.inst_root == (std::vector<uint32_t>{1, 0, 1, 0}));
    uint32_t w;
    memcpy(&w, &fp.inst_trav[0].row[0][3], 4);
    CHECK(w == 1);
}

template<class T> std::string sha(const std::vector<T>& v)
{
    ptgref::Sha256 h;
    h.update(v.data(), v.size() * sizeof(T));
    return h.hex();
}

// The real scene as tools/walk_sim packs it: frame 0 committed, then the frame under test.
int real_scene(const char* assets)
{
    ptg_render_config cfg;
    ptg_render_config_default(&cfg);
    cfg.width = 1280; cfg.height = 720; cfg.samples_per_pixel = 1024;
    ptg_scene* scene = nullptr;
    if(ptg_scene_load(assets, &cfg, &scene)) { fprintf(stderr, "%s\n", ptg_last_error()); return 1; }
    BlockCache c;
    for(uint32_t frame: {0u, 450u, 1400u})
    {
        if(ptg_scene_setup_frame(scene, frame)) { fprintf(stderr, "%s\n", ptg_last_error()); return 1; }
        ptg_scene_view v;
        ptg_scene_view_get(scene, &v);
        if(frame == 0)
            c.set_scene(v.nodes, v.links, v.static_node_count, v.indices, v.index_count, v.pos, v.albedo, v.material, v.vertex_count);
        FramePack fp;
        std::string err;
        if(c.pack_frame(v.subframes, v.subframe_count, v.instances, v.instance_count, v.nodes + v.static_node_count,
                        v.links + 8 * v.static_node_count, v.static_node_count, v.node_count - v.static_node_count, fp, err))
        { fprintf(stderr, "frame %u: %s\n", frame, err.c_str()); return 1; }
        size_t all = 0, one = 0, none = 0, tri0 = 0;
        for(const InstBox& b: fp.inst_box)
        {
            (b.sub == kInstAllSubframes ? all : b.sub == kInstNoCandidate ? none : one)++;
            tri0 += b.tri_count == 0;
        }
        printf("frame %u: instances %zu subframes %zu all %zu one %zu never %zu tri0 %zu jobs %zu\n", frame, v.instance_count,
               v.subframe_count, all, one, none, tri0, fp.mesh_jobs.size());
        printf("frame %u inst_trav %s\nframe %u inst_shade %s\nframe %u inst_box %s\nframe %u mesh_jobs %s\n", frame,
               sha(fp.inst_trav).c_str(), frame, sha(fp.inst_shade).c_str(), frame, sha(fp.inst_box).c_str(), frame,
               sha(fp.mesh_jobs).c_str());
        if(frame == 0) c.commit(fp);
    }
    ptg_scene_destroy(scene);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if(argc == 3 && !strcmp(argv[1], "real")) return real_scene(argv[2]);
    test_classes();
    test_named_twice();
    test_leaf_box_gate();
    test_failed_frame();
    test_mesh_jobs();
    printf("%s\n", g_failed ? "records_test: FAILED" : "records_test: all passed");
    return g_failed ? 1 : 0;
}
