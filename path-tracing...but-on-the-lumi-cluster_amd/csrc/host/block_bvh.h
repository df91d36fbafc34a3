// Host packer of the block BVH records (device/block_format.h) and of the
// per-instance records (device/records.h): the host half of the uploads.
#pragma once
#include "ptg.h"
#include "../device/block_format.h"
#include "../device/records.h"
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace ptg {

unsigned host_threads();   // scene.cpp: this process's share of the host's CPUs

struct BlockBvh {
    uint32_t root = 0;          // root block index (absolute: block_base + position)
    uint32_t blocks = 0;        // blocks appended
    uint32_t stack_entries = 0; // most stack entries a walk of this BVH can hold
    uint32_t max_payload = 0;   // largest leaf payload
};

// Packs one BVH given in the reference layout - nodes[0..count) and the eight
// link orders links[o * count + i] (bvh.cc:195-229) - appending its blocks
// (kBlockCopies copies each, one per octant) to `out`.  Child block
// indices are block_base + position in `out` / kBlockCopies.  Checked, with an error in `err`:
//   - the links are the reference builder's: a tree rooted at node 0 whose
//     every order lists each node's children forward, or reversed when the
//     octant's sign on the node's axis is not positive (bvh.cc:173-191);
//   - every box contains its children's boxes (the walk skips inner boxes);
//   - leaf payloads are below payload_limit (and 2^28).
bool pack_block_bvh(const ptg_bvh_node* nodes, const ptg_bvh_link* links, uint32_t count, uint32_t block_base,
                    uint32_t payload_limit, std::vector<BlockCopy>& out, BlockBvh& info, std::string& err);

// Whether every leaf box of a BLAS (nodes[0..count), links in the reference
// layout) is exactly the bounds of its triangle's three positions as the
// reference's builder computes them (bvh.cc:243-246: fmin / fmax, the float
// overloads, whose tie rule fixes the sign of zero bounds) - the any-hit
// walk tests a candidate triangle's leaf box from its vertices
// (BlockWalker::try_candidate).  `indices` and `pos` are the scene's arrays;
// the mesh is (index_offset, triangle_count, base_vertex_offset).  Built by
// the host compiler with the builder's flags (host/hmath.h), so the
// comparison is bit for bit: hipcc's std::fmin (llvm.minnum) may pick either
// zero of a +0 / -0 tie.
bool leaf_boxes_are_vertex_bounds(const ptg_bvh_node* nodes, const ptg_bvh_link* links, uint32_t count,
                                  const uint32_t* indices, size_t index_count, const ptg_float3* pos, size_t vertex_count,
                                  uint32_t index_offset, uint32_t triangle_count, uint32_t base_vertex_offset);

// A packed BLAS in the block cache.
struct BlasRecord {
    uint32_t root = 0;          // root block
    uint32_t count = 0;         // node count it was packed with
    uint32_t max_payload = 0;   // largest triangle index its leaves name
};

// What one frame upload writes: the blocks it adds to the block buffer
// [BLAS blocks][TLAS blocks], the per-instance records, and the meshes whose
// triangle records the device still has to pack.
struct FramePack {
    uint32_t blas_base = 0;                 // block index of new_blas[0]
    uint32_t tlas_base = 0;                 // block index of tlas[0]
    std::vector<BlockCopy> new_blas;       // BLASes no earlier frame packed
    std::vector<BlockCopy> tlas;           // this frame's TLASes, one per subframe
    std::unordered_map<uint32_t, BlasRecord> new_records;
    std::vector<uint32_t> tlas_root;        // per subframe
    std::vector<uint32_t> inst_root;        // per instance: its BLAS's root block
    uint32_t blas_stack = 0, tlas_stack = 0;
    std::vector<InstTrav> inst_trav;       // per instance (device/records.h)
    std::vector<InstShade> inst_shade;
    std::vector<InstBox> inst_box;
    std::vector<MeshJob> mesh_jobs;        // meshes no committed frame packed, by first appearance
    std::unordered_set<uint32_t> new_mesh; // their index_offsets
    uint32_t total_blocks() const { return tlas_base + uint32_t(tlas.size() / kBlockCopies); }
    uint32_t stack_bound() const { return blas_stack + tlas_stack; }   // stack entries a walk can hold
};

// The host half of ptg_upload_scene and ptg_upload_frame, kept free of device
// code so the CPU tests (tools/walk_sim.cpp, tests/frame_records) run exactly
// what the uploads run: a host copy of the static scene, the BLAS blocks
// packed so far, and the packing of a frame's handles into blocks and
// per-instance records.
struct BlockCache {
    // the static scene (set_scene): the BLAS nodes + links in reference layout
    // (packed into blocks when an instance first names a BLAS) and the mesh
    // arrays the occluder candidates' leaf boxes are checked against
    std::vector<ptg_bvh_node> nodes;
    std::vector<ptg_bvh_link> links;
    std::vector<uint32_t> indices;
    std::vector<ptg_float3> pos;
    bool attrs_finite = false;                            // every vertex albedo / material value finite
    // per (BLAS, mesh): every BLAS leaf's box is its triangle's vertex bounds
    // (bvh.cc:243-246), so a candidate triangle's leaf box can be computed from
    // its vertices (k_wf_walk<ANY>); checked once per pair (a memo of a pure
    // function of the scene: pack_frame fills it)
    mutable std::map<std::tuple<uint32_t, uint32_t, uint32_t>, bool> leaf_bounds_ok;
    std::vector<BlockCopy> blas;                         // committed BLAS blocks
    std::unordered_map<uint32_t, BlasRecord> records;     // BLAS node_offset -> record
    uint32_t blas_stack = 0;                              // largest committed BLAS stack bound
    std::unordered_set<uint32_t> packed_mesh;             // index_offsets of the meshes whose triangle records are on the device

    // Forgets the scene and everything packed from it.
    void clear();
    // Replaces the static scene: copies the arrays (may throw std::bad_alloc)
    // and scans the vertex attributes for attrs_finite.  Nothing packed from
    // the previous scene survives.
    void set_scene(const ptg_bvh_node* scene_nodes, const ptg_bvh_link* scene_links, size_t node_count,
                   const uint32_t* scene_indices, size_t index_count, const ptg_float3* scene_pos,
                   const ptg_float4* albedo, const ptg_float4* material, size_t vertex_count);
    // Checks every handle of the frame (BLAS and mesh ranges, TLAS ranges,
    // leaf payloads, block links), packs the BLASes not yet cached plus every
    // subframe's TLAS, and fills the per-instance records and the mesh jobs.
    // `frame_nodes/links` are the frame's TLAS arrays (reference layout)
    // starting at global node `first_node`.  Returns PTG_OK, or PTG_E_RANGE
    // with the reason in `err`; the cache is not modified (leaf_bounds_ok aside).
    int pack_frame(const ptg_subframe* subframes, size_t subframe_count, const ptg_tlas_instance* instances,
                   size_t instance_count, const ptg_bvh_node* frame_nodes, const ptg_bvh_link* frame_links,
                   size_t first_node, size_t frame_node_count, FramePack& fp, std::string& err) const;
    // What a frame packs joins the cache here and nowhere else, after every
    // upload of it succeeded: its new BLASes, their records and stack bound,
    // and its new meshes.  An upload that fails half-way never leaves the
    // cache claiming records that were not written.
    void commit(const FramePack& fp);
};

} // namespace ptg
