// What every HIP unit of libptg.so needs from the context (host side):
// pt_kernels.hip (the path tracer and the context's life cycle), image_ops.hip
// (the image-space filters) and upload.hip (the scene and frame upload).
//
//   DevBuf, HostStage     a device buffer and a pinned staging buffer
//   struct ptg_context    one struct, its fields grouped by the unit that uses them
//   fail, hip_fail, PTG_HIP, bind, grid_for, launch_plain
//
// Everything is inline and in namespace ptg: one definition, no unit owns a copy.
#pragma once
#include <hip/hip_runtime.h>
#include "ptg.h"
#include "device/layout.h"
#include "device/ref_math.h"   // CS_COUNT
#include "host/block_bvh.h"
#include <algorithm>
#include <string>
#include <vector>

namespace ptg {

void set_last_error(const std::string& msg);   // scene.cpp

constexpr int kBlock = 256;
constexpr uint32_t kWfSlots = 2;           // concurrent wavefront chunk pipelines (ptg_context::Slot)
constexpr int kRedoWords = 2 + dm::CS_COUNT;    // the certified shading's redo tallies (pt_kernels.hip, tally_redo)
constexpr uint32_t kTemporalMaxCams = 512;  // ptg_temporal_accumulate_clamped's n_cams

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { if(p) (void)hipFree(p); }
    hipError_t reserve(size_t n)
    {
        if(n <= bytes && p) return hipSuccess;
        if(p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if(n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, n);
        if(e == hipSuccess) bytes = n;
        return e;
    }
    template<typename T> T* as() const { return static_cast<T*>(p); }
};

// Pinned host staging for asynchronous uploads; `done` marks the end of the
// copies that last read it.
struct HostStage {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    ~HostStage()
    {
        if(done)
        {
            (void)hipEventSynchronize(done);
            (void)hipEventDestroy(done);
        }
        if(p) (void)hipHostFree(p);
    }
    // waits for the copies that last read it, then grows it to n bytes
    hipError_t reserve(size_t n)
    {
        if(!done)
            if(hipError_t e = hipEventCreateWithFlags(&done, hipEventDisableTiming)) return e;
        if(hipError_t e = hipEventSynchronize(done)) return e;
        if(n <= bytes && p) return hipSuccess;
        if(p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipHostMalloc(&p, std::max<size_t>(n, 1), hipHostMallocDefault);
        if(e == hipSuccess) bytes = std::max<size_t>(n, 1);
        return e;
    }
};

inline int hip_fail(hipError_t e, const char* what)
{
    set_last_error(std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
    return PTG_E_HIP;
}

#define PTG_HIP(call)                                                        \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if(e_ != hipSuccess) return hip_fail(e_, #call);                     \
    } while(0)

inline int fail(int code, const std::string& msg)
{
    set_last_error(msg);
    return code;
}

inline uint32_t grid_for(size_t n, uint32_t block = kBlock) { return uint32_t((n + block - 1) / block); }

} // namespace ptg

struct ptg_context {
    // ---- every unit ----
    int device = 0;
    hipStream_t stream = nullptr;
    ptg::DevBuf tmp_a, tmp_b, tmp_c;       // scratch of the host-pointer entries (parity entries, ptg_tonemap)

    // ---- written by the upload unit, read by the render unit ----
    // static scene: the shading arrays in reference layout and the triangle
    // records
    ptg::DevBuf indices, pos, normal, albedo, material, tris, tri_shade;
    // the host's copy of the scene and everything packed from it so far
    // (host/block_bvh.h; the BLAS blocks' device copy leads `blocks`)
    ptg::BlockCache cache;
    size_t blas_on_device = 0;                           // leading cache.blas entries already in `blocks`
    bool scene_ready = false;
    // frame: blocks = [BLAS blocks][this frame's TLAS blocks]
    ptg::DevBuf blocks, tlas_root, subframes, inst_trav, inst_shade, inst_box, jobs, polygon;
    ptg::HostStage stage[2];                             // ptg_upload_frame's pinned staging, used alternately
    uint32_t stage_next = 0;
    size_t block_count = 0, subframe_count = 0, instance_count = 0;
    uint32_t stack_bound = 0;                            // TLAS + BLAS stack bound of this frame (entries)
    std::vector<uint32_t> host_tlas_root;
    std::vector<uint32_t> host_tri_base;                 // per instance: its mesh's first triangle (TraceOut names mesh-global triangles)
    bool frame_ready = false;

    // ---- the image-space unit ----
    ptg::DevBuf dn_a, dn_b;                // ptg_denoise: the demodulated image and its ping-pong partner
    ptg::DevBuf tp_cams;                   // ptg_temporal_accumulate_clamped: the call's cameras (kTemporalMaxCams TemporalCam)
    ptg::HostStage tp_stage[2];            // their pinned staging, used alternately
    uint32_t tp_stage_next = 0;

    // ---- the render unit ----
    bool counting = false;
    // render workspace
    ptg::DevBuf spill;                     // the walk stacks' spill areas, per (slot, walk kind)
    ptg::DevBuf acc, counters;
    ptg::DevBuf mom;                       // ptg_render_moments: the running (s1, s2, n) per pixel, beside acc
    ptg::DevBuf feat_acc;                  // ptg_render_with_features: the eight running feature sums per pixel (k_fold_features)
    ptg::DevBuf feat_spill;                // ptg_render_features: the walk stacks' spill areas
    ptg::DevBuf walk_state;                // ptg_walk_rays: its queue, path state, results and statistics
    ptg::DevBuf ad_list, ad_count;         // ptg_render_adaptive: the active pixels' ids and their number
    uint32_t ad_passes_run = 0;            // ptg_last_adaptive_stats
    uint64_t ad_active[16] = {};
    ptg::DevBuf debug;                     // PTG_DEBUG builds: kDebugSlots violation counters
    uint64_t last_counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // k_trace launch timing (HIP events on the launch stream)
    bool timing = false;
    std::vector<hipEvent_t> ev_start, ev_stop;
    std::vector<int> ev_kind;
    size_t ev_used = 0;
    // 0: wavefront pipeline (default), 1: megakernel
    int pipeline = 0;
    uint32_t persistent_blocks = 2048;
    uint32_t walk_grid[2] = {2048, 2048};
    uint32_t walk_xcds[2] = {1, 1};        // XCDs the walk grid is dealt over (8 when the grid divides evenly)
    uint32_t walk_lds[2] = {0, 0};         // dynamic LDS per walk block: cold state + stack rings, padded to cap residency
    uint32_t hbm_pct = 35;                 // wavefront state: at most this share of HBM per chunk pipeline (ptg_set_hbm_share)
    // wavefront: <= 2^chunk_log2 live paths per chunk.  2^27 paths x 380 B
    // (kStateBytesPerPath 364 + the 16 B sample) = 51 GB per pipeline, ~35% of an MI355X's HBM for the two pipelines
    // together, so a default render leaves most of the GPU to other tenants;
    // 2^28 (~71%) is 1-3% faster on a GPU the renderer owns alone.
    uint32_t chunk_log2 = 27;
    uint64_t kind_counters[6][8] = {};
    uint64_t walk_stats[2][8] = {};        // counting builds: WalkStat tallies of the closest-hit / any-hit walks
    uint64_t redo_stats[ptg::kRedoWords] = {};  // counting builds: the certified shading's redo tallies (tally_redo)
    // Wavefront chunk pipelines ("slots").  With two slots, consecutive
    // chunks run concurrently on their own stream pairs and buffers, so one
    // chunk's round-0 walk and shade overlap the other's sky and shadow
    // kernels; k_accumulate still folds the chunks in sample order, each on
    // its chunk's slot stream, chained by events across the slots (fold_chunk).
    // The megakernel and concurrency levels 0 / 1 use slot 0 alone.
    struct Slot {
        // main: the slot's first camera, closest-hit walk, classify, shade,
        // fold; side: shadow walk, sky and the camera of the slot's next chunk
        // (trace_chunk_wavefront).  Slot 0 has no main stream of its own: its
        // chunks run on the caller's stream (main_of)
        hipStream_t main = nullptr, side = nullptr;
        // the events that order main and side; ev_acc: the slot's last fold done
        hipEvent_t ev_main = nullptr, ev_side = nullptr, ev_acc = nullptr;
        ptg::DevBuf state, samples;   // path state (SlotState), the chunk's per-sample results
        ptg::DevBuf feat;             // a fused render's per-sample features: two arrays laid out like `samples`
    };
    Slot slot[ptg::kWfSlots];
    hipStream_t main_of(uint32_t k) const { return k ? slot[k].main : stream; }
    uint32_t concurrency = 2;              // ptg_set_concurrency
    hipEvent_t ev_render_start = nullptr;
    hipEvent_t ev_first_camera = nullptr;  // a render's first camera kernels take turns (trace_chunk_wavefront)

    ~ptg_context()
    {
        for(Slot& b: slot)
        {
            for(hipEvent_t e: {b.ev_main, b.ev_side, b.ev_acc})
                if(e) (void)hipEventDestroy(e);
            for(hipStream_t st: {b.main, b.side})
                if(st) (void)hipStreamDestroy(st);
        }
        if(ev_render_start) (void)hipEventDestroy(ev_render_start);
        if(ev_first_camera) (void)hipEventDestroy(ev_first_camera);
        for(hipEvent_t e: ev_start) (void)hipEventDestroy(e);
        for(hipEvent_t e: ev_stop) (void)hipEventDestroy(e);
    }

    // Wait for everything queued on the context's streams: the caller's
    // stream and every slot's own.
    hipError_t drain() const
    {
        for(uint32_t k = 0; k < ptg::kWfSlots; ++k)
            for(hipStream_t st: {main_of(k), slot[k].side})
                if(hipError_t e = hipStreamSynchronize(st)) return e;
        return hipSuccess;
    }
    // Grow a workspace buffer.  Growing frees the old allocation, which work
    // still queued on the context's streams may read: drain them first (rare,
    // the buffers only grow), rather than rely on hipFree's implicit sync.
    hipError_t grow(ptg::DevBuf& b, size_t n) const
    {
        if(n <= b.bytes && b.p) return hipSuccess;
        if(b.p)
            if(hipError_t e = drain()) return e;
        return b.reserve(n);
    }

    ptg::DevScene scene_args(const ptg_render_config* cfg) const
    {
        using namespace ptg;
        DevScene s;
        s.blocks = blocks.as<BlockCopy>();
        s.tlas_root = tlas_root.as<uint32_t>();
        s.tris = tris.as<TriRec>();
        s.tri_shade = tri_shade.as<TriShade>();
        s.inst_trav = inst_trav.as<InstTrav>();
        s.inst_shade = inst_shade.as<InstShade>();
        s.inst_box = inst_box.as<InstBox>();
        s.indices = indices.as<uint32_t>();
        s.normal = normal.as<float>();
        s.albedo = albedo.as<float>();
        s.material = material.as<float>();
        s.subframes = subframes.as<uint8_t>();
        s.polygon = polygon.as<float2>();
        s.width = cfg ? cfg->width : 0;
        s.height = cfg ? cfg->height : 0;
        s.spp = cfg ? cfg->samples_per_pixel : 0;
        s.max_bounces = cfg ? cfg->max_bounces : 0;
        s.student_id = cfg ? cfg->student_id : 0;
        s.blur_step = cfg ? cfg->samples_per_motion_blur_step : 8;
        s.subframe_count = uint32_t(subframe_count);
        s.block_count = uint32_t(block_count);
        s.spill = nullptr;
        s.spill_stride = stack_bound;
        s.tri_count = uint32_t(cache.indices.size() / 3);
        s.inst_count = uint32_t(instance_count);
        s.debug = PTG_DEBUG ? debug.as<uint32_t>() : nullptr;
        s.attrs_finite = cache.attrs_finite ? 1u : 0u;
        return s;
    }
};

namespace ptg {

inline int bind(ptg_context* ctx)
{
    if(!ctx) return fail(PTG_E_INVALID, "null context");
    PTG_HIP(hipSetDevice(ctx->device));
    return PTG_OK;
}

// A launch outside the render path's timed and counted ones, on ctx->stream,
// its launch error checked (ptg_last_kernel_times lists the render path
// alone).  `blocks` of kBlock work-items: grid_for(n) for one per element.
template<typename... P, typename... A>
int launch_plain(ptg_context* ctx, uint32_t blocks, void (*kernel)(P...), const A&... args)
{
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, args...);
    PTG_HIP(hipGetLastError());
    return PTG_OK;
}

} // namespace ptg
