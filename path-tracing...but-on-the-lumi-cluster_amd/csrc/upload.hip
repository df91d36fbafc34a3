// The scene and frame upload of the C ABI (include/ptg.h): the device half of
// what host/block_bvh.cpp packs, and the two kernels that finish the records
// on the device.
//
//   k_polygon_table every subframe's aperture polygon vertices, from the camera's own polygon_vertex
//   k_pack_tris     indices + positions -> TriRec (48 B / triangle), + vertex attributes -> TriShade (128 B)
//   (BVH blocks are packed on the host, host/block_bvh.cpp)
//
// device/path_tracer.h is included for polygon_vertex and the subframe field
// readers (rd_f, rd_u) alone: the table must hold the bits camera_ray would
// compute.  Nothing else of the walker or the shading is used, and the
// wavefront pipeline is not included.
//
// No fallback path exists: every entry point fails loudly (negative code +
// ptg_last_error) when HIP or the device is unavailable.
#include "runtime.h"
#include "device/path_tracer.h"
#include <cstring>
#include <new>

using namespace ptg;
using namespace ptg::dm;

namespace {

// ---------------------------------------------------------------- kernels --

// The aperture polygon's vertex directions of every subframe (regular_polygon,
// path_tracer.hh:50-62): (sin, cos) of side_radians * k + angle for
// k = 0 .. sides + 1.  A polygon has few vertices and every sample's camera
// ray uses two of them, so the camera kernel reads them instead of making
// four double-precision trig calls.  One thread per (subframe, k).
__global__ void k_polygon_table(const uint8_t* __restrict__ subframes, uint32_t count, float2* __restrict__ out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= count * kPolyStride) return;
    const uint32_t i = t / kPolyStride, k = t % kPolyStride;
    const uint8_t* cam = subframes + size_t(i) * SF_STRIDE + SF_CAM;
    const int32_t sides = (int32_t)rd_u(cam, 80);
    f2 v{0.0f, 0.0f};
    if(sides > 3 && (uint32_t)sides <= kPolyMaxSides && k <= (uint32_t)sides + 1u)
        v = polygon_vertex(rd_f(cam, 76), (uint32_t)sides, (float)k);
    out[t] = make_float2(v.x, v.y);
}

// one thread per triangle of each new mesh: its TriRec (positions) and its
// TriShade (normals, albedos, materials), both at index_offset / 3 + t
__global__ void k_pack_tris(const uint32_t* __restrict__ indices, const float4* __restrict__ pos, TriRec* __restrict__ out,
                            const MeshJob* __restrict__ jobs, const float4* __restrict__ normal,
                            const float4* __restrict__ albedo, const float4* __restrict__ material,
                            TriShade* __restrict__ shade)
{
    const MeshJob j = jobs[blockIdx.y];
    for(uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < j.triangle_count; t += gridDim.x * blockDim.x)
    {
        const uint32_t* tri = indices + j.index_offset + 3u * t;
        const float4 a = pos[j.base_vertex_offset + tri[0]];
        const float4 b = pos[j.base_vertex_offset + tri[1]];
        const float4 c = pos[j.base_vertex_offset + tri[2]];
        TriRec r;
        r.p0x = a.x; r.p0y = a.y; r.p0z = a.z; r.p1x = b.x;
        r.p1y = b.y; r.p1z = b.z; r.p2x = c.x; r.p2y = c.y;
        r.p2z = c.z; r.pad0 = 0; r.pad1 = 0; r.pad2 = 0;
        out[j.index_offset / 3u + t] = r;
        TriShade sh;
        for(int k = 0; k < 3; ++k)
        {
            const uint32_t v = j.base_vertex_offset + tri[k];
            const float4 n = normal[v], a = albedo[v], m = material[v];
            float* g = sh.v + 10 * k;
            g[0] = n.x; g[1] = n.y; g[2] = n.z;
            g[3] = a.x; g[4] = a.y; g[5] = a.z;
            g[6] = m.x; g[7] = m.y; g[8] = m.z; g[9] = m.w;
        }
        sh.v[30] = sh.v[31] = 0.0f;
        shade[j.index_offset / 3u + t] = sh;
    }
}

} // namespace

extern "C" {

int ptg_upload_scene(ptg_context* ctx, const ptg_bvh_node* nodes, const ptg_bvh_link* links, size_t node_count,
                     const uint32_t* indices, size_t index_count, const ptg_float3* pos, const ptg_float3* normal,
                     const ptg_float4* albedo, const ptg_float4* material, size_t vertex_count)
{
    if(int r = bind(ctx)) return r;
    if(!nodes || !links || !indices || !pos || !normal || !albedo || !material || node_count == 0 || index_count % 3)
        return fail(PTG_E_INVALID, "ptg_upload_scene: bad arguments");
    if(node_count >= (1u << 28) / 8 || index_count >= (1u << 31) || vertex_count >= (1u << 31))
        return fail(PTG_E_RANGE, "ptg_upload_scene: scene too large for 32-bit indexing");
    ctx->scene_ready = ctx->frame_ready = false;
    ctx->blas_on_device = 0;
    try
    {
        ctx->cache.set_scene(nodes, links, node_count, indices, index_count, pos, albedo, material, vertex_count);
    }
    catch(const std::bad_alloc&)
    {
        return fail(PTG_E_NOMEM, "ptg_upload_scene: host copy of the BVH nodes");
    }
    PTG_HIP(ctx->indices.reserve(index_count * 4));
    PTG_HIP(ctx->pos.reserve(vertex_count * 16));
    PTG_HIP(ctx->normal.reserve(vertex_count * 16));
    PTG_HIP(ctx->albedo.reserve(vertex_count * 16));
    PTG_HIP(ctx->material.reserve(vertex_count * 16));
    // the walks address triangle records by 32-bit byte offsets (BlockWalker::leaf_select)
    if(index_count / 3 * sizeof(TriRec) + 128 > 0xFFFFFFFFull)
        return fail(PTG_E_RANGE, "triangle records above 4 GB (" + std::to_string(index_count / 3) + " triangles)");
    // slack: the walk's leaf phase reads a triangle as four 16-byte rows (the
    // 48-byte record and the next 16 bytes)
    PTG_HIP(ctx->tris.reserve(std::max<size_t>(1, index_count / 3) * sizeof(TriRec) + 128));
    PTG_HIP(ctx->tri_shade.reserve(std::max<size_t>(1, index_count / 3) * sizeof(TriShade)));
    hipStream_t s = ctx->stream;
    PTG_HIP(hipMemcpyAsync(ctx->indices.p, indices, index_count * 4, hipMemcpyHostToDevice, s));
    PTG_HIP(hipMemcpyAsync(ctx->pos.p, pos, vertex_count * 16, hipMemcpyHostToDevice, s));
    PTG_HIP(hipMemcpyAsync(ctx->normal.p, normal, vertex_count * 16, hipMemcpyHostToDevice, s));
    PTG_HIP(hipMemcpyAsync(ctx->albedo.p, albedo, vertex_count * 16, hipMemcpyHostToDevice, s));
    PTG_HIP(hipMemcpyAsync(ctx->material.p, material, vertex_count * 16, hipMemcpyHostToDevice, s));
    PTG_HIP(hipStreamSynchronize(s));
    ctx->scene_ready = true;
    return PTG_OK;
}

namespace {

// The body of ptg_upload_frame (which adds the C ABI's exception barrier).
int upload_frame(ptg_context* ctx, const ptg_subframe* subframes, size_t subframe_count, const ptg_tlas_instance* instances,
                 size_t instance_count, const ptg_bvh_node* frame_nodes, const ptg_bvh_link* frame_links, size_t first_node,
                 size_t frame_node_count)
{
    ctx->frame_ready = false;
    hipStream_t s = ctx->stream;

    // Validate every handle, pack the BLASes no earlier frame named plus
    // this frame's TLASes, and build the per-instance records and the mesh
    // jobs (host/block_bvh.cpp, checked there before any kernel can follow a
    // block link).  What this call packs joins the cache only at the commit
    // below.
    FramePack fp;
    std::string err;
    if(int r = ctx->cache.pack_frame(subframes, subframe_count, instances, instance_count, frame_nodes, frame_links,
                                     first_node, frame_node_count, fp, err))
        return fail(r, "ptg_upload_frame: " + err);
    const std::vector<MeshJob>& mesh_jobs = fp.mesh_jobs;

    // Device copies, asynchronous: everything the frame uploads is gathered
    // into one of two pinned staging buffers and copied on the context's
    // stream, behind the render already queued there - the host returns at
    // once and the next render queues right behind the copies.  A staging
    // buffer is reused only after its copies of two uploads ago completed.
    // Growing a device buffer frees the old one, which an in-flight render
    // may still read: the context's streams are drained first (rare).
    auto grow = [&](DevBuf& b, size_t n) { return ctx->grow(b, n); };
    // blocks = [BLAS blocks][TLAS blocks]; growing the buffer drops the BLAS
    // blocks already there, which are then uploaded again
    const std::vector<BlockCopy>& old_blas = ctx->cache.blas;
    const size_t blas_total = old_blas.size() + fp.new_blas.size();
    const size_t need = (blas_total + fp.tlas.size()) * sizeof(BlockCopy);
    if(need > 0xFFFFFFFFull)   // the walks address blocks by 32-bit byte offsets (BlockWalker::block_rows)
        return fail(PTG_E_RANGE, "block records above 4 GB (" + std::to_string(need) + " B)");
    if(need > ctx->blocks.bytes)
    {
        PTG_HIP(grow(ctx->blocks, need + need / 8));
        ctx->blas_on_device = 0;
    }
    PTG_HIP(grow(ctx->tlas_root, subframe_count * sizeof(uint32_t)));
    PTG_HIP(grow(ctx->inst_trav, instance_count * sizeof(InstTrav)));
    PTG_HIP(grow(ctx->inst_shade, instance_count * sizeof(InstShade)));
    PTG_HIP(grow(ctx->inst_box, instance_count * sizeof(InstBox)));
    PTG_HIP(grow(ctx->subframes, subframe_count * sizeof(ptg_subframe)));
    PTG_HIP(grow(ctx->polygon, subframe_count * kPolyStride * sizeof(float2)));
    if(!mesh_jobs.empty()) PTG_HIP(grow(ctx->jobs, mesh_jobs.size() * sizeof(MeshJob)));
    BlockCopy* dev = ctx->blocks.as<BlockCopy>();
    struct Part { const void* src; size_t n; void* dst; };
    std::vector<Part> parts;
    if(ctx->blas_on_device < old_blas.size())
        parts.push_back({old_blas.data() + ctx->blas_on_device, (old_blas.size() - ctx->blas_on_device) * sizeof(BlockCopy),
                         dev + ctx->blas_on_device});
    parts.push_back({fp.new_blas.data(), fp.new_blas.size() * sizeof(BlockCopy), dev + old_blas.size()});
    parts.push_back({fp.tlas.data(), fp.tlas.size() * sizeof(BlockCopy), dev + blas_total});
    parts.push_back({fp.tlas_root.data(), subframe_count * sizeof(uint32_t), ctx->tlas_root.p});
    parts.push_back({fp.inst_trav.data(), instance_count * sizeof(InstTrav), ctx->inst_trav.p});
    parts.push_back({fp.inst_shade.data(), instance_count * sizeof(InstShade), ctx->inst_shade.p});
    parts.push_back({fp.inst_box.data(), instance_count * sizeof(InstBox), ctx->inst_box.p});
    parts.push_back({subframes, subframe_count * sizeof(ptg_subframe), ctx->subframes.p});
    parts.push_back({mesh_jobs.data(), mesh_jobs.size() * sizeof(MeshJob), ctx->jobs.p});
    size_t total = 0;
    for(const Part& q: parts) total += (q.n + 255) & ~size_t(255);
    HostStage& hs = ctx->stage[ctx->stage_next];
    ctx->stage_next ^= 1u;
    PTG_HIP(hs.reserve(total));
    size_t off = 0;
    for(const Part& q: parts)
    {
        if(q.n == 0) continue;
        char* h = static_cast<char*>(hs.p) + off;
        memcpy(h, q.src, q.n);
        PTG_HIP(hipMemcpyAsync(q.dst, h, q.n, hipMemcpyHostToDevice, s));
        off += (q.n + 255) & ~size_t(255);
    }
    PTG_HIP(hipEventRecord(hs.done, s));
    hipLaunchKernelGGL(k_polygon_table, dim3(grid_for(subframe_count * kPolyStride)), dim3(kBlock), 0, s,
                       ctx->subframes.as<uint8_t>(), uint32_t(subframe_count), ctx->polygon.as<float2>());
    PTG_HIP(hipGetLastError());
    if(!mesh_jobs.empty())
    {
        uint32_t maxt = 0;
        for(const MeshJob& j: mesh_jobs) maxt = std::max(maxt, j.triangle_count);
        dim3 grid(std::min<uint32_t>(grid_for(maxt), 4096), uint32_t(mesh_jobs.size()));
        hipLaunchKernelGGL(k_pack_tris, grid, dim3(kBlock), 0, s, ctx->indices.as<uint32_t>(), ctx->pos.as<float4>(),
                           ctx->tris.as<TriRec>(), ctx->jobs.as<MeshJob>(), ctx->normal.as<float4>(),
                           ctx->albedo.as<float4>(), ctx->material.as<float4>(), ctx->tri_shade.as<TriShade>());
        PTG_HIP(hipGetLastError());
    }

    // every upload is queued: what this call packed joins the cache
    ctx->cache.commit(fp);
    ctx->blas_on_device = ctx->cache.blas.size();
    ctx->block_count = fp.total_blocks();
    ctx->stack_bound = fp.stack_bound();
    ctx->host_tlas_root = fp.tlas_root;
    ctx->host_tri_base.resize(instance_count);
    for(size_t i = 0; i < instance_count; ++i) ctx->host_tri_base[i] = fp.inst_shade[i].index_offset / 3;
    ctx->subframe_count = subframe_count;
    ctx->instance_count = instance_count;
    ctx->frame_ready = true;
    return PTG_OK;
}

} // namespace

int ptg_upload_frame(ptg_context* ctx, const ptg_subframe* subframes, size_t subframe_count,
                     const ptg_tlas_instance* instances, size_t instance_count, const ptg_bvh_node* frame_nodes,
                     const ptg_bvh_link* frame_links, size_t first_node, size_t frame_node_count)
{
    if(int r = bind(ctx)) return r;
    if(!ctx->scene_ready) return fail(PTG_E_INVALID, "ptg_upload_frame: upload the scene first");
    if(!subframes || !subframe_count || !instances || !instance_count || !frame_nodes || !frame_links || !frame_node_count)
        return fail(PTG_E_INVALID, "ptg_upload_frame: bad arguments");
    if(first_node != ctx->cache.nodes.size())
        return fail(PTG_E_INVALID, "ptg_upload_frame: first_node must equal the uploaded static node count");
    if(first_node + frame_node_count >= (1ull << 31)) return fail(PTG_E_RANGE, "ptg_upload_frame: too many nodes");
    try
    {
        return upload_frame(ctx, subframes, subframe_count, instances, instance_count, frame_nodes, frame_links, first_node,
                            frame_node_count);
    }
    catch(const std::bad_alloc&)
    {
        ctx->frame_ready = false;
        return fail(PTG_E_NOMEM, "ptg_upload_frame: host memory");
    }
}

int ptg_upload_from_scene(ptg_context* ctx, const ptg_scene* scene, int include_static)
{
    ptg_scene_view v;
    if(int r = ptg_scene_view_get(scene, &v)) return r;
    if(include_static)
        if(int r = ptg_upload_scene(ctx, v.nodes, v.links, v.static_node_count, v.indices, v.index_count, v.pos, v.normal,
                                    v.albedo, v.material, v.vertex_count))
            return r;
    return ptg_upload_frame(ctx, v.subframes, v.subframe_count, v.instances, v.instance_count, v.nodes + v.static_node_count,
                            v.links + 8 * v.static_node_count, v.static_node_count, v.node_count - v.static_node_count);
}

} // extern "C"
