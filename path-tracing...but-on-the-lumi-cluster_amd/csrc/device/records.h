// The per-triangle and per-instance records of the device-side data layout
// (layout.h, DESIGN.md "Data layout in HBM"), free of HIP types: the host
// compiler includes this header too (host/block_bvh.cpp fills the
// per-instance records and the mesh jobs of a frame upload).
#pragma once
#include <stdint.h>

namespace ptg {

struct alignas(16) TriRec {
    float p0x, p0y, p0z, p1x;
    float p1y, p1z, p2x, p2y;
    float p2z, pad0, pad1, pad2;
};
static_assert(sizeof(TriRec) == 48, "TriRec is three 16-byte loads");

// TriShade 128 B: what the shading of a hit on triangle t of a mesh reads
// (path_tracer.hh:373-392: three indices, then each vertex's normal, albedo
// and material), gathered once per mesh at tri_shade[index_offset/3 + t]:
// vertex k's normal xyz, albedo xyz and material xyzw at floats 10k..10k+9,
// then 2 pad floats - eight 16-byte loads of one 128-byte line instead of
// three index loads and nine dependent gathers.
struct alignas(16) TriShade {
    float v[32];
};
static_assert(sizeof(TriShade) == 128, "TriShade is one 128-byte line");

struct alignas(16) InstTrav {
    // row k = inv_transform.r[k].{x,y,z} in [0..2]; [3] = the bits of the
    // BLAS's root block, the mesh's triangle base, 0, 0 for rows 0..3: four
    // whole, aligned 16-byte loads (the device reads the rows as float4)
    float row[4][4];
};
static_assert(sizeof(InstTrav) == 64, "InstTrav is four 16-byte loads");

struct alignas(16) InstShade {
    float rot[9];              // transform.r[k].{x,y,z} for k = 0..2
    uint32_t index_offset, base_vertex_offset, pad[5];
};
static_assert(sizeof(InstShade) == 64, "InstShade is four 16-byte loads");

// InstBox 32 B: an instance's TLAS leaf box (the reference's leaf node, the
// bounds of its transformed BLAS root box, bvh.cc:259-281) and where it is a
// leaf: the any-hit walk's occluder candidates (k_wf_walk<ANY>) test an
// instance's leaf box directly, without walking the TLAS down to it.
//   lo.xyz, w = sub: the one subframe whose TLAS holds the instance, or
//                    kInstAllSubframes (every TLAS holds it, with this same box),
//                    or kInstNoCandidate (neither: never a candidate)
//   hi.xyz, w = the triangle count of its mesh (candidate triangles are below it)
struct alignas(16) InstBox {
    float lo[3];
    uint32_t sub;
    float hi[3];
    uint32_t tri_count;
};
static_assert(sizeof(InstBox) == 32, "InstBox is two 16-byte loads");
constexpr uint32_t kInstAllSubframes = 0xFFFFFFFFu, kInstNoCandidate = 0xFFFFFFFEu;

// A mesh whose TriRec / TriShade records k_pack_tris still has to write.
struct MeshJob {
    uint32_t index_offset, triangle_count, base_vertex_offset, pad;
};
static_assert(sizeof(MeshJob) == 16, "MeshJob is one 16-byte load");

} // namespace ptg
