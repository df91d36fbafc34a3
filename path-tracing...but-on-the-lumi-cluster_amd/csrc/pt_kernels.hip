// The path tracer: its HIP kernels, the render driver, the context's life
// cycle and knobs, and their part of the C ABI (include/ptg.h).  The
// image-space filters are image_ops.hip, the scene and frame upload is
// upload.hip; runtime.h holds what the three share.
//
//   k_wf_camera<COUNT, MAP>, k_wf_walk<ANY, COUNT>, k_wf_classify,
//   k_wf_shade<COUNT, MP, FEAT>, k_wf_sky<COUNT, FEAT>
//                   the wavefront pipeline (device/wavefront.h)
//   k_trace         path_trace_pixel for a (pixel set x sample chunk) grid,
//                   one work-item per (pixel, sample); results to a
//                   [sample][pixel] float4 buffer in HBM
//   k_accumulate<MOMENTS>  baseline_render's j-ordered float32 sum over the chunk,
//                   then (last chunk) / SPP + tonemap_pixel (main.cc:24-43);
//                   <true> keeps the samples' luminance moments too
//   k_sample_list   path_trace_pixel for an explicit (x, y, j) list (parity)
//   k_rays          ray_query closest hit + shadow any-hit (parity)
//   k_camera_rays   camera_ray's first ray per (pixel, sample) (parity)
//   k_scatter_tiles
//   k_assemble_tile_packs  a frame's five planes from a tile shard's gathered
//                   packs in one launch (ptg_assemble_tile_packs)
//   k_features     first-hit albedo, normal and depth
//   k_fold_features the same sums from the features round 0 of a fused render
//                   stored per sample (ptg_render_with_features: k_wf_shade /
//                   k_wf_sky with FEAT), folded beside k_accumulate
//   k_ad_select<ALL>, k_ad_fold
//                   adaptive sampling (ptg_render_adaptive): the stopping rule
//                   compacted into a pixel list, the fold over that list (its
//                   camera is k_wf_camera over AdaptivePass)
//   k_resolve<PER_PIXEL>  the deferred resolve: running sums divided and
//                   tonemapped outside a fold - ptg_render_adaptive's final
//                   division by each pixel's own count, and ptg_accum_resolve,
//                   which does not end the accumulation (the folds of both
//                   are k_ad_fold / k_accumulate and k_fold_features)
//
// A frame's five planes and the three sums they are closed from travel as
// Planes and Sums (host/planes.h); the closing arithmetic is
// device/image_math.h's close_*.
//
// No fallback path exists: every entry point fails loudly (negative code +
// ptg_last_error) when HIP or the device is unavailable.
#include "runtime.h"
#include "host/planes.h"
#include "device/image_math.h"
#include "device/path_tracer.h"
#include "device/wavefront.h"
#include "ptg_device.h"   // ptg_device_selftest, compiled here with the library's own flags (ptg_arith_selftest)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <unordered_map>

using namespace ptg;
using namespace ptg::dm;

namespace {

#define PTG_SHADE_WAVES 3   // the certified pass (MathFast): 168 VGPRs, 6 spilled; the exact pass runs at 2
// the surface pass's math: MathFast (certified ocml + the exact redo pass) or
// MathExactLds (glibc's algorithms directly, no redo)
using ShadeMath = MathFast;

// ---------------------------------------------------------------- kernels --

// Which image pixels a launch covers: a rectangle, or an interleaved tile set.
struct PixelMap {
    uint32_t tiles;                 // 0: rectangle, 1: tiles
    uint32_t x0, y0, w, h;          // rectangle
    uint32_t tw, th, tiles_x, first, stride;
    uint32_t img_w, img_h;
    uint32_t npix;

    __device__ __forceinline__ bool pixel(uint32_t p, uint32_t& x, uint32_t& y) const
    {
        if(!tiles)
        {
            x = x0 + p % w;
            y = y0 + p / w;
            return true;
        }
        const uint32_t per = tw * th;
        const uint32_t t = first + (p / per) * stride;
        const uint32_t q = p % per;
        x = (t % tiles_x) * tw + q % tw;
        y = (t / tiles_x) * th + q / tw;
        return x < img_w && y < img_h;
    }
    // local sample index -> sample index of the frame (k_wf_camera's MAP)
    __device__ __forceinline__ uint32_t sample(uint32_t j) const { return j; }
};

// 16-byte non-temporal load / store of a float4 or uint4 record
template<typename T> __device__ __forceinline__ T nt_load(const T* p)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
    T out;
    __builtin_memcpy(&out, &v, 16);
    return out;
}
template<typename T> __device__ __forceinline__ void nt_store(T* p, T value)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v4u v;
    __builtin_memcpy(&v, &value, 16);
    __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(p));
}

__device__ __forceinline__ unsigned long long wave_sum(uint32_t v)
{
    unsigned long long s = v;
    for(int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// Counting builds only: wave-reduce the counters, one atomic per counter per wave.
__device__ __forceinline__ void flush_counters(const Counters& c, unsigned long long* dev, uint32_t samples)
{
    const unsigned long long v[8] = {wave_sum(samples), wave_sum(c.visits), wave_sum(c.tri_tests),
                                     wave_sum(c.blas_entries), wave_sum(c.queries), wave_sum(c.shades),
                                     wave_sum(c.tlas_visits), wave_sum(c.iters)};
    if((threadIdx.x & 63u) == 0)
        for(int k = 0; k < 8; ++k)
            if(v[k]) atomicAdd(dev + k, v[k]);
}

// Counting builds: paths the MathFast shading passes listed for the exact
// pass - [0] surface, [1] sky - then per certificate site (ref_math.h
// CertSite) the listed paths in which it failed (kRedoWords words).
__device__ __forceinline__ void tally_redo(unsigned long long* tally, int kind, uint32_t fail_mask)
{
    atomicAdd(tally + kind, 1ull);
    for(int k = 0; k < CS_COUNT; ++k)
        if(fail_mask & (1u << k)) atomicAdd(tally + 2 + k, 1ull);
}

// ---- wavefront pipeline (csrc/device/wavefront.h) ----


// Lane -> (pixel, sample) of a chunk: a wave holds 8 pixels x 8 consecutive
// samples (one motion-blur subframe); consecutive waves walk the sample
// groups of one pixel group.
__device__ __forceinline__ void chunk_coords(uint32_t i, uint32_t nj, uint32_t& p, uint32_t& jj)
{
    const uint32_t wave = i >> 6, lane = i & 63u;
    const uint32_t sgroups = (nj + 7u) >> 3;
    jj = (wave % sgroups) * 8u + (lane & 7u);
    p = (wave / sgroups) * 8u + (lane >> 3);
}

// counts[2r]: paths queued for round r; counts[2r+1]: their pending NEE rays.
// Round 0 is every lane of the chunk in lane order (queue position = lane, no
// compaction); lanes outside the chunk or the image are queued as dead paths
// (an empty TLAS, retired by the first shade).  The camera writes path state
// and counts[0] only, never the slot's sample buffer: a hoisted camera runs
// before the fold of the chunk ahead of it has read that buffer
// (trace_chunk_wavefront), so a dead lane's zero sample is written where the
// dead path retires (shade_path).
// MAP says which pixels and samples the queue holds: npix queue pixels,
// pixel(p, x, y) (false: a dead lane) and sample(j), the frame's sample index
// of local sample j.  PixelMap: a rectangle or tile set, every sample.
// AdaptivePass: a pass's pixel list and its strided samples; the queue
// positions, PathSoA records and dead lanes are the same, so the walk,
// classify, shade and sky kernels run on either queue unchanged.
template<bool COUNT, class MAP>
__global__ __launch_bounds__(kBlock) void k_wf_camera(DevScene sc, MAP pm, uint32_t j0, uint32_t nj, uint32_t M,
                                                      PathSoA S, uint32_t* __restrict__ counts,
                                                      unsigned long long* __restrict__ counters)
{
    if(blockIdx.x == 0 && threadIdx.x == 0) counts[0] = M;
    uint32_t lives = 0;
    for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x)
    {
        uint32_t p, jj, x = 0, y = 0;
        chunk_coords(i, nj, p, jj);
        const bool in_chunk = p < pm.npix && jj < nj;
        const bool live = in_chunk && pm.pixel(p, x, y);
        const uint32_t slot = in_chunk ? jj * pm.npix + p : 0xFFFFFFFFu;
        if(!live)
        {
            st_state(S.meta + i, make_uint4(slot, META_DEAD, kBePop, 0u));   // no TLAS: the walk ends at once
            st_state(S.ray_o + i, make_float4(0.f, 0.f, 0.f, 0.f));
            st_state(S.ray_d + i, make_float4(0.f, 0.f, 1.f, 0.f));
            continue;
        }
        const int32_t j = (int32_t)pm.sample(j0 + jj);
        const uint8_t* sf = subframe_of(sc, j);
        u4 seed;
        f3 o, d;
        camera_ray(sc, sf, x, y, j, seed, o, d);
        const uint32_t sub = (uint32_t)(sf - sc.subframes) / SF_STRIDE;
        st_state(S.meta + i, make_uint4(slot, meta_pack(0, false, sub), sc.tlas_root[sub], 0u));
        st_state(S.seed + i, to_uint4(seed));
        st_state(S.ray_o + i, make_float4(o.x, o.y, o.z, 0.f));
        st_state(S.ray_d + i, make_float4(d.x, d.y, d.z, 0.f));
        ++lives;
    }
    if(COUNT) flush_counters(Counters{}, counters, lives);
}

// BVH walks of one round over a queue: ANY = false walks the extension rays
// (closest hit, queue positions 0..n-1), ANY = true the pending NEE rays
// (any hit, positions from the NEE list).  Persistent "while-while" loop:
// the grid is sized to what is resident, each wave owns a contiguous range of
// the queue (no atomics), and a lane that finishes its ray takes the next one
// of its wave's range, so the wave never idles behind its longest ray.
#ifndef PTG_ANY_RUN
#define PTG_ANY_RUN 4
#endif
constexpr uint32_t kAnyRun = PTG_ANY_RUN;   // consecutive queue groups per run of the any-hit walk (k_wf_walk)
constexpr int kRefillIdle = 24;   // refill once at least this many lanes are idle (16 / 32: slower)
// waves per SIMD the walks are compiled for: the closest-hit walk at 96 VGPRs
// (104 uncapped, no spills at 96), the any-hit walk at 80 (76 used), so a
// shade wave (160) fits beside it
#define PTG_WALK_WAVES 5
#define PTG_SHADOW_WAVES 6
#define PTG_WALK_ATTR __attribute__((amdgpu_waves_per_eu(ANY ? PTG_SHADOW_WAVES : PTG_WALK_WAVES, 8)))
constexpr int kWalkUnroll = 2;     // node steps per leaf phase (1 and 3 measured slower)
// Walk residency per walk kind (closest hit, any hit): the LDS of a walk
// block is padded to 1 / kWalkResident of the CU's (0: not padded), and the
// grid holds kWalkBlocksPerCu blocks per CU (one resident wave, see
// ptg_context_create).  Timing knobs PTG_WALK_RESIDENT[_ANY] and
// PTG_WALK_BLOCKS[_ANY] override them (the results do not depend on them).
constexpr uint32_t kWalkResident[2] = {4, 0};
constexpr uint32_t kWalkBlocksPerCu[2] = {3, 3};
constexpr uint32_t kBands = 1024;   // XCD bands of a walk queue: a multiple of the XCD count (8 on MI355X)
// a chunk's device counters: per round the queue / NEE list lengths (2 words,
// plus 4 spare), the hit / sky list lengths (2), the redo list lengths (2)
constexpr uint32_t kCountWords(uint32_t rounds) { return 4 * (rounds + 2) + 2 * rounds; }
// a chunk pipeline's state bytes per queued path: 2 ping-pong PathSoA halves
// of 9 x 16 B, 2 TraceOut sets (hit 16 B, bary 8 B, shadow 4 B), 5 lists of
// 4 B (2 NEE lists, hit, sky, redo); the chunk sizing budgets with it and
// carve_slot_state checks it against the fields it hands out
constexpr size_t kStateBytesPerPath = 2 * 9 * 16 + 2 * (16 + 8 + 4) + 5 * 4;
// the path state of one chunk pipeline (ptg_context::Slot::state).  A chunk
// whose round 0 reads half S[p] uses S[(p + r) & 1] as round r's `cur` and the
// other half as its `nxt`; its last round appends no survivors, so the half
// S[(p + rounds) & 1] is free once round `rounds - 2` has been shaded, and the
// slot's next chunk takes it as its round-0 half: its camera kernel can run
// beside this chunk's last round (trace_chunk_wavefront).  That camera also
// zeroes and starts the next chunk's counters while this chunk's are in use,
// hence two blocks of them, alternating per chunk.  TraceOut sets and NEE
// lists go by the round's own parity: the camera touches neither.
struct SlotState {
    PathSoA S[2];
    TraceOut trs[2];   // per round parity: the sky kernel of round r reads its set while round r+1 writes the other
    uint32_t* lists[2];                 // NEE lists, by round parity
    uint32_t *hit_list, *sky_list;      // this round's paths by shading kernel
    uint32_t* redo_hit;                 // surface paths to shade again with MathExact
    uint32_t* counts[2];                // kCountWords(rounds) words each, by chunk parity on the slot
};
constexpr size_t slot_state_bytes(size_t M, uint32_t rounds) { return M * kStateBytesPerPath + 2 * kCountWords(rounds) * 4 + 256; }
// Cuts a slot's state buffer (slot_state_bytes(M, rounds) at `base`) into its
// arrays of M entries, in this order in memory, the two counts blocks behind
// them (kCountWords is even: both stay 8-byte aligned for the packed atomics).
// False if the fields' bytes per path are not kStateBytesPerPath.
inline bool carve_slot_state(char* base, size_t M, uint32_t rounds, SlotState& t)
{
    size_t per_path = 0;
    auto take = [&](auto*& field) {
        using T = std::remove_reference_t<decltype(*field)>;
        field = reinterpret_cast<T*>(base + per_path * M);
        per_path += sizeof(T);
    };
    for(PathSoA& s: t.S)
    {
        take(s.meta); take(s.seed); take(s.ray_o); take(s.ray_d); take(s.att);
        take(s.contrib); take(s.batt); take(s.nee_c); take(s.nee_d);
    }
    for(TraceOut& o: t.trs) { take(o.hit); take(o.bary); take(o.shadow); }
    take(t.lists[0]); take(t.lists[1]); take(t.hit_list); take(t.sky_list); take(t.redo_hit);
    t.counts[0] = reinterpret_cast<uint32_t*>(base + per_path * M);
    t.counts[1] = t.counts[0] + kCountWords(rounds);
    return per_path == kStateBytesPerPath;
}
constexpr uint32_t kRedoGrid = 16;   // blocks of the MathExact shading passes (grid-stride over a short list)

// Walk statistics of the counting build (per walk kind, see WalkStats): how
// many lanes each vector-memory instruction of the walk serves.  The walk's
// vector-memory issue costs the same per wave instruction whatever its EXEC
// mask (profiles/r02_probe/ta_probe.txt), so lanes per instruction is the
// lever on that level.
enum WalkStat : int { WS_NODE_WAVES = 0, WS_NODE_LANES, WS_LEAF_WAVES, WS_LEAF_LANES, WS_REFILL_WAVES,
                      WS_REFILL_LANES, WS_ITERS, WS_ACTIVE_LANES, WS_COUNT };
// Behind a walk kind's WS_COUNT words, per walk rather than per instruction
// (ptg_walk_rays returns them; ptg_last_walk_stats keeps to the first
// WS_COUNT): walks started; walks whose stack size passed the LDS window
// (size() > kCap after a node phase, so part of the stack went to HBM and, in
// the closest-hit walk, came back); the largest stack size seen, in the
// stack's own units (LdsStack: entries, LdsSlotStack: slots); any-hit walks
// that took the wave's candidate.  Tallied in k_wf_walk from outside the stack structs.
enum WalkExtra : int { WX_STARTED = 0, WX_PAST_WINDOW, WX_MAX_SIZE, WX_CANDIDATES, WX_COUNT };
constexpr int kWalkWords = WS_COUNT + WX_COUNT;   // a walk kind's words of wstats

template<bool ANY, bool COUNT>
__global__ __launch_bounds__(kBlock) PTG_WALK_ATTR void k_wf_walk(DevScene sc, PathSoA S, const uint32_t* __restrict__ counts,
                                                    uint32_t round, const uint32_t* __restrict__ list, TraceOut tr,
                                                    uint32_t nxcd, unsigned long long* __restrict__ counters,
                                                    unsigned long long* __restrict__ wstats)
{
    // the walks wait on memory most of their cycles: when a walk wave and a
    // shade / sky wave of the other pipeline are both ready on a SIMD, the
    // walk issues first (priorities 1-3 measured; 3: frame 0 -0.2%, frame
    // 450 -0.3%, profiles/r04m_prio/)
    __builtin_amdgcn_s_setprio(3);
    const uint32_t n = counts[2 * round + (ANY ? 1 : 0)];
    const uint32_t lane = threadIdx.x & 63u;
    // XCD-aware static split: the queue's 64-entry groups (8 pixels x 8
    // samples each) are cut into kBands bands dealt round-robin to the XCDs
    // (workgroup b runs on XCD b % nxcd), so each XCD's L2 serves a few image
    // bands instead of the whole frame.  Inside its bands, wave w of an XCD
    // takes the groups w, w + W, w + 2W, ...: every wave samples all of its
    // XCD's bands (balanced) and the waves in flight cover a narrow window.
    const uint32_t xcd = blockIdx.x % nxcd;
    const uint32_t waves = ((gridDim.x / nxcd) * blockDim.x) >> 6;
    // (the same for a wave's 64 lanes: in a scalar register, and with it the
    // wave's range of the queue and its cursor, so the refill test at the top
    // of every iteration is a scalar compare)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(((blockIdx.x / nxcd) * blockDim.x + threadIdx.x) >> 6);
    const uint32_t groups = (n + 63u) >> 6;
    const uint32_t band = max(1u, (groups + kBands - 1u) / kBands);
    const uint32_t local = (kBands / nxcd) * band;    // this XCD's group slots (some past the end)
    // The any-hit walk deals runs of kAnyRun consecutive groups per wave (wave
    // w: runs w, w + W, ...) instead of single groups: a wave's next group is
    // then usually the same pixels' next 8 samples (or the next pixels), so
    // the occluder its last group found (the candidate, try_candidate) lies on
    // the new rays' way to the sun too.  The closest-hit walk keeps runs of 1.
    // Runs only where they keep a run inside one band and still leave every
    // wave work (small queues - late rounds, small frames, tile renders - take
    // single groups: a run crossing bands would jump nxcd * band groups).
    static_assert((kAnyRun & (kAnyRun - 1u)) == 0, "kAnyRun is a power of two");
    const uint32_t rl = (ANY && band >= kAnyRun && groups >= waves * kAnyRun) ? uint32_t(__builtin_ctz(kAnyRun)) : 0u;
    const uint32_t R = 1u << rl;
    const uint32_t runs = (local + R - 1u) >> rl;
    const uint32_t end = wave < runs ? ((runs - wave + waves - 1) / waves) * R * 64u : 0u;
    uint32_t cursor = 0;
    const float tmin = (ANY || round > 0) ? MIN_RAY_DIST : 0.0f;
    const float tmax = ANY ? MAX_RAY_DIST : 1e9f;
    const float tmin_p = __uint_as_float(__float_as_uint(tmin) + 1u);   // BlockWalker::tmin_next() of every walk here
    Counters cnt;
    // LDS: every lane's world ray, then the stack windows, one 64-lane x kCap
    // entry table per wave (ptg_context_create sizes the block's LDS)
    extern __shared__ WalkCold cold[];
    BlockWalker<LdsCold, typename WalkStackOf<ANY>::type> w;
    w.cold.c = (lds_cold_t*)(&cold[threadIdx.x]);   // C cast: generic -> LDS address space
    w.st.bind(cold + blockDim.x, threadIdx.x >> 6, lane, sc.spill + (size_t(blockIdx.x) * blockDim.x + threadIdx.x) * sc.spill_stride);
    bool active = false;
    uint32_t q = 0;
    // ANY: the wave's latest occluder (instance, triangle), wave-uniform (in
    // scalar registers): the candidate its next rays try first
    // (BlockWalker::try_candidate; a wave's rays come from one 8-pixel x
    // 8-sample group at a time, their shadow rays are nearly parallel)
    uint32_t occ_inst = 0xFFFFFFFFu, occ_prim = 0;
    // a finished walk writes its result: the shadow flag, or the closest hit;
    // results stream once through the caches (non-temporal), so they do not
    // evict BVH records from L2 / the Infinity Cache
    auto finish = [&](int r) {
        if(ANY) __builtin_nontemporal_store(r == 2 ? 1u : 0u, tr.shadow + q);
        else
        {
            const Hit h = w.result();
            // (primitive_id: the mesh-global triangle, LdsCold::kGlobalTri)
            nt_store(tr.hit + q, make_uint4(__float_as_uint(h.thit), h.instance_id, h.primitive_id, h.back_face ? 1u : 0u));
            if(h.instance_id != 0xFFFFFFFFu)   // a miss is shaded without its barycentrics
                __builtin_nontemporal_store(__builtin_bit_cast(unsigned long long, make_float2(h.bx, h.by)),
                                            reinterpret_cast<unsigned long long*>(tr.bary + q));
        }
    };
    unsigned long long ws[WS_COUNT] = {};   // COUNT: lane 0's tallies for its wave
    uint32_t wx[WX_COUNT] = {};             // COUNT: this lane's per-walk tallies (WalkExtra)
    bool past_window = false;               // COUNT: this lane's walk has been counted in WX_PAST_WINDOW
    auto tally = [&](int waves_slot, bool loads) {
        const unsigned long long m = __ballot(loads);
        if(lane == 0 && m)
        {
            ws[waves_slot] += 1;
            ws[waves_slot + 1] += (unsigned long long)__popcll(m);
        }
    };
    for(;;)
    {
        if(cursor < end)
        {
            const unsigned long long idle = __ballot(!active);
            const uint32_t nidle = (uint32_t)__popcll(idle);
            if(nidle >= (uint32_t)kRefillIdle || nidle == 64u)
            {
                bool took = false;
                if(!active)
                {
                    const uint32_t v = cursor + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                    const uint32_t k = v >> 6;   // this wave's k-th group
                    const uint32_t l = (wave + (k >> rl) * waves) * R + (k & (R - 1u));
                    const uint32_t t = ((xcd + nxcd * (l / band)) * band + l % band) * 64u + (v & 63u);
                    if(v < end && l < local && t < n)
                    {
                        q = ANY ? list[t] : t;
#if PTG_DEBUG
                        // the NEE list names positions of this round's path queue
                        const bool bad = ANY && q >= counts[2 * round];
                        if(bad && sc.debug) atomicAdd(sc.debug + kDebugQueue, 1u);
                        if(!bad)
#endif
                        {
                            // path state streams once through the caches: non-temporal
                            const uint4 m = nt_load(S.meta + q);
#if PTG_DEBUG
                            debug_check_round(sc, m, round);
#endif
                            w.init(m.z, xyz(nt_load(S.ray_o + q)),
                                   ANY ? xyz(nt_load(S.nee_d + q)) : xyz(nt_load(S.ray_d + q)), tmin, tmax);
                            if(ANY) w.try_candidate(sc, occ_inst, occ_prim, meta_sub(m));
                            active = true;
                            took = true;
                            if(COUNT)
                            {
                                cnt.queries++;
                                wx[WX_STARTED]++;
                                past_window = false;
                                if(ANY && w.pend != kBePop) wx[WX_CANDIDATES]++;
                            }
                        }
                    }
                }
                if(COUNT) tally(WS_REFILL_WAVES, took);
                cursor = min(end, cursor + nidle);
            }
        }
        if(!__any(active)) break;
        if(COUNT)
        {
            const unsigned long long m = __ballot(active);
            if(lane == 0)
            {
                ws[WS_ITERS] += 1;
                ws[WS_ACTIVE_LANES] += (unsigned long long)__popcll(m);
                cnt.iters++;
            }
        }
        // Node phase, up to kWalkUnroll block steps (each after the pop it
        // needs), for lanes not standing at a leaf; then one leaf phase for the
        // lanes that are.  The leaf code (triangle test, BLAS entry) then runs
        // once per iteration with many lanes, not once per block step with few.
        int r = 0;
        // A walk that ends in any phase of this iteration only leaves
        // `active`; the one finish site after the leaf phase writes its
        // result (q and the walk's best hit stay as they are until the next
        // refill, at the top of the next iteration).
        const bool was_active = active;
#pragma unroll
        for(int u = 0; u < kWalkUnroll; ++u)
        {
            if(COUNT) cnt.step_loads = 0;
            if(active && !w.at_leaf()) r = w.template node_step<COUNT>(sc, cnt, tmin_p);   // (a lane with a parked triangle walks on)
            if(COUNT) tally(WS_NODE_WAVES, (cnt.step_loads & 1u) != 0);
            if(active && r != 0)
            {   // ANY: after a candidate's instance, the TLAS (BlockWalker::resume_tlas)
                if(!(ANY && w.resume_tlas()))
                {
                    active = false;
                }
                r = 0;
            }
        }
        if(COUNT && active)
        {
            const uint32_t size = w.st.size();
            wx[WX_MAX_SIZE] = max(wx[WX_MAX_SIZE], size);
            if(size > decltype(w.st)::kCap && !past_window)
            {
                past_window = true;
                wx[WX_PAST_WINDOW]++;
            }
        }
        if(COUNT) cnt.step_loads = 0;
        bool occluded = false;
        if(active && w.wants_leaf())
        {
            r = w.template leaf_step<ANY, COUNT>(sc, cnt);
            occluded = ANY && r == 2;
            if(r != 0) active = false;
        }
        if(was_active && !active) finish(occluded ? 2 : 1);
        if(ANY)
        {   // the wave's candidate becomes an occluder one of its lanes just found
            const unsigned long long om = __ballot(occluded);
            if(om)
            {
                const int l = __ffsll((long long)om) - 1;
                occ_inst = __builtin_amdgcn_readlane(w.inst, l);
                occ_prim = __builtin_amdgcn_readlane(w.cur, l);   // a walk that returned 2 left its occluder in cur
            }
        }
        if(COUNT) tally(WS_LEAF_WAVES, (cnt.step_loads & 6u) != 0);
    }
    if(COUNT)
    {
        flush_counters(cnt, counters, 0);
        if(lane == 0)
            for(int k = 0; k < WS_COUNT; ++k)
                if(ws[k]) atomicAdd(wstats + k, ws[k]);
        unsigned long long largest = wx[WX_MAX_SIZE];
        for(int o = 32; o > 0; o >>= 1) largest = max(largest, (unsigned long long)__shfl_xor(largest, o));
        for(int k = 0; k < WX_COUNT; ++k)
        {
            const unsigned long long v = k == WX_MAX_SIZE ? largest : wave_sum(wx[k]);
            if(lane != 0 || !v) continue;
            if(k == WX_MAX_SIZE) atomicMax(wstats + WS_COUNT + k, v);
            else atomicAdd(wstats + WS_COUNT + k, v);
        }
    }
}

// Shading of one round is split by what the paths will run.
//
// k_wf_classify reads every queued path's trace result and deals the queue,
// 256 entries per block, into two lists through an LDS counting sort: paths
// whose ray hit a surface (shaded by k_wf_shade) and paths whose ray left the
// scene (shaded by k_wf_sky), each grouped by whether a pending NEE ray still
// has to be finished.  A wave then runs one of the long, mutually exclusive
// branches of shade_path, and the sky branch - the double-precision
// atmosphere integrals - runs in its own small kernel at high occupancy.
// Which lane shades which path has no effect on the result.
__global__ __launch_bounds__(kBlock) void k_wf_classify(const uint32_t* __restrict__ counts, uint32_t round, TraceOut tr,
                                                        uint32_t* __restrict__ hit_list,
                                                        uint32_t* __restrict__ sky_list, uint32_t* __restrict__ lcounts)
{
    // Each block deals a tile of kTile entries with ONE 64-bit atomic on the
    // packed (hit, sky) list lengths: a device-scope atomic is a fabric round
    // trip serialized per address, so their number, not the bytes, sets this
    // kernel's time.
    constexpr uint32_t kSub = 8, kTile = kSub * kBlock;
    const uint32_t n = counts[2 * round];
    __shared__ uint32_t bin_count[4];
    __shared__ unsigned long long base2;
    for(uint32_t tile = blockIdx.x * kTile; tile < n; tile += gridDim.x * kTile)
    {
        if(threadIdx.x < 4) bin_count[threadIdx.x] = 0;
        __syncthreads();
        uint32_t key[kSub], rank[kSub];
#pragma unroll
        for(uint32_t k = 0; k < kSub; ++k)
        {
            const uint32_t q = tile + k * kBlock + threadIdx.x;
            key[k] = 4u;
            rank[k] = 0;
            if(q < n)
            {
                const bool hit = __uint_as_float(tr.hit[q].x) > 0.0f;
                // shade(round-1) wrote 1 for survivors without a pending NEE ray,
                // the shadow walk 0/1 for those with one (meta is not read)
                const bool nee = round > 0 && tr.shadow[q] == 0;
                key[k] = (hit ? 2u : 0u) | (nee ? 1u : 0u);
                rank[k] = atomicAdd(&bin_count[key[k]], 1u);
            }
        }
        __syncthreads();
        if(threadIdx.x == 0)
        {
            const unsigned long long nsky = bin_count[0] + bin_count[1], nhit = bin_count[2] + bin_count[3];
            base2 = atomicAdd(reinterpret_cast<unsigned long long*>(lcounts), (nsky << 32) | nhit);
        }
        __syncthreads();
        const uint32_t hit_base = uint32_t(base2), sky_base = uint32_t(base2 >> 32);
#pragma unroll
        for(uint32_t k = 0; k < kSub; ++k)
        {
            const uint32_t q = tile + k * kBlock + threadIdx.x;
            if(key[k] == 4u) continue;
            if(key[k] & 2u) hit_list[hit_base + (key[k] == 3u ? bin_count[2] : 0u) + rank[k]] = q;
            else sky_list[sky_base + (key[k] == 1u ? bin_count[0] : 0u) + rank[k]] = q;
        }
        __syncthreads();   // bin_count is rewritten by the next tile
    }
}

// MISS: the caller shades a path whose ray left the scene (k_wf_classify put
// it on the sky list because its hit distance was not positive).  The walk
// reports such a ray as WalkerT::result() does, thit = -1 and no hit, and the
// sky branch of shade_path reads nothing else of it: the hit and barycentric
// records are not fetched (nor the barycentrics written by the walk).
template<bool MISS = false>
__device__ __forceinline__ void load_queued(const PathSoA& cur, const TraceOut& tr, uint32_t q, PathRec& p, Hit& h,
                                            bool& occluded, bool carried)
{
    p = load_path(cur, q, carried);
    occluded = meta_nee(p.meta) ? tr.shadow[q] != 0 : false;
    if(MISS)
    {
        h.thit = -1.0f;
        h.instance_id = 0xFFFFFFFFu;
        h.primitive_id = 0;
        h.back_face = false;
        h.bx = h.by = h.bz = 0.0f;
        return;
    }
    const uint4 hv = ld_state(tr.hit + q);
    // (bz = 1 - bx - by, the same float arithmetic as the walk's result())
    const float2 bv = __builtin_bit_cast(float2, __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(tr.bary + q)));
    h.thit = __uint_as_float(hv.x);
    h.instance_id = hv.y;
    h.primitive_id = hv.z;
    h.back_face = hv.w != 0;
    h.bx = bv.x; h.by = bv.y; h.bz = 1.0f - bv.x - bv.y;
}

// A shading kernel's math policy (ref_math.h); MathExactLds copies glibc
// exp's table into the kernel's LDS array first (every thread, before any
// returns).
template<class MP>
__device__ __forceinline__ MP shading_policy(glibc::u2v* exp_tab)
{
    MP mp;
    if constexpr(MP::kLdsExp)
    {
        glibc::exp_table_to_lds((glibc::lds_u2v_t*)exp_tab);   // C cast: generic -> LDS address space
        __syncthreads();
        mp.xt = glibc::ExpTabLds{(const glibc::lds_u2v_t*)exp_tab};
    }
    (void)exp_tab;
    return mp;
}

// Surface hits: NEE finish, bounce tail, then NEE setup + BSDF sample of the
// next bounce or retire.  Survivors are appended per block (one atomic per
// queue per block), stored contiguously and grouped by the octant of their
// next ray, so the next round's 64-ray groups mostly walk one link order.
// MP = MathFast: ocml's double library with rounding certificates (ref_math.h);
// a path whose certificate failed is listed in redo_list (its length in
// redo_count) and shaded again by the MathExact instance, which takes
// redo_list as its hit_list (and appends nothing to a redo list).
// FEAT: round 0 of a fused render (ptg_render_with_features); every path also
// stores its first-hit features (shade_path).  Every other launch, the
// MathExact pass of that round included, is the FEAT = false instantiation.
template<bool COUNT, class MP, bool FEAT = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MP::kFast ? PTG_SHADE_WAVES : 2, 8))) void k_wf_shade(
    DevScene sc, PathSoA cur, PathSoA nxt, uint32_t* __restrict__ counts, uint32_t round, TraceOut tr,
    const uint32_t* __restrict__ hit_list, const uint32_t* __restrict__ lcounts, uint32_t* __restrict__ next_list,
    uint32_t* __restrict__ next_shadow, float4* __restrict__ out, uint32_t* __restrict__ redo_list,
    uint32_t* __restrict__ redo_count, unsigned long long* __restrict__ counters, unsigned long long* __restrict__ redo_tally,
    FeatOut<FEAT> feat)
{
    const uint32_t n = lcounts[0];
    Counters cnt;
    __shared__ uint32_t oct_count[8], oct_start[8], blk_base, nee_total, nee_base;
    __shared__ glibc::u2v exp_tab[MP::kLdsExp ? glibc::kExpTabEntries : 1];
    const MP mp0 = shading_policy<MP>(exp_tab);
    for(uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x)
    {
        const uint32_t i = base + threadIdx.x;
        bool cont = false, nee = false;
        PathRec p;
#if PTG_DEBUG
        const bool bad_q = i < n && hit_list[i] >= counts[2 * round];
        if(bad_q && sc.debug) atomicAdd(sc.debug + kDebugList, 1u);
        if(i < n && !bad_q)
#else
        if(i < n)
#endif
        {
            Hit h;
            bool occluded;
            const uint32_t q = hit_list[i];
            load_queued(cur, tr, q, p, h, occluded, !FEAT && round > 0);
#if PTG_DEBUG
            debug_check_round(sc, p.meta, round);
#endif
            MP mp = mp0;
            const ShadeResult res = shade_path<COUNT, 1, MP, FEAT>(sc, p, h, occluded, out, cnt, mp, feat);
            if(MP::kFast && res == SH_REDO)
            {
                redo_list[atomicAdd(redo_count, 1u)] = q;
                if(COUNT) tally_redo(redo_tally, 0, mp.fail_mask);
            }
            cont = res == SH_CONTINUE;
            nee = cont && meta_nee(p.meta);
        }
        if(threadIdx.x < 8) oct_count[threadIdx.x] = 0;
        if(threadIdx.x == 8) nee_total = 0;
        __syncthreads();
        const uint32_t okey = cont ? octant(p.ray_d) : 0u;
        const uint32_t orank = cont ? atomicAdd(&oct_count[okey], 1u) : 0u;
        const uint32_t nrank = nee ? atomicAdd(&nee_total, 1u) : 0u;
        __syncthreads();
        if(threadIdx.x == 0)
        {   // one 64-bit atomic on the packed (queue, NEE list) lengths
            unsigned long long total = 0;
            for(int k = 0; k < 8; ++k) { oct_start[k] = uint32_t(total); total += oct_count[k]; }
            const unsigned long long old =
                (total | nee_total)
                    ? atomicAdd(reinterpret_cast<unsigned long long*>(&counts[2 * (round + 1)]),
                                (uint64_t(nee_total) << 32) | total)
                    : 0ull;
            blk_base = uint32_t(old);
            nee_base = uint32_t(old >> 32);
        }
        __syncthreads();
        const uint32_t qn = blk_base + oct_start[okey] + orank;
        if(cont) store_path(nxt, qn, p);
        if(nee) next_list[nee_base + nrank] = qn;
        else if(cont) __builtin_nontemporal_store(1u, next_shadow + qn);   // no NEE ray: k_wf_classify reads "occluded"
        __syncthreads();   // the LDS tables are rewritten by the next iteration
    }
    if(COUNT) flush_counters(cnt, counters, 0);
}

// Rays that left the scene: sun disk, NEE finish, the atmosphere integrals
// (path_tracer.hh:456-588), retire.  No survivors.  The atmosphere is exp
// work end to end, and here glibc's restated exp (its table copied to LDS)
// beats ocml's plus rounding certificates (MathFast: 2x the code, spills at
// 5 waves; measured DESIGN.md section 4), so this pass is exact by itself.
#define PTG_SKY_WAVES 5     // 96 VGPRs (10 spilled); 4 waves: 103, none - 5 measured 0.26% faster on frames 0 and 450 (profiles/r04q_tune/ab_sky5.log)
// FEAT as in k_wf_shade: a fused render's round 0 stores the miss features too.
template<bool COUNT, bool FEAT = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PTG_SKY_WAVES, 8))) void k_wf_sky(
    DevScene sc, PathSoA cur, TraceOut tr, uint32_t round, const uint32_t* __restrict__ sky_list,
    const uint32_t* __restrict__ lcounts, float4* __restrict__ out, unsigned long long* __restrict__ counters,
    FeatOut<FEAT> feat)
{
    const uint32_t n = lcounts[1];
    Counters cnt;
    __shared__ glibc::u2v exp_tab[glibc::kExpTabEntries];
    MathExactLds mp = shading_policy<MathExactLds>(exp_tab);
    for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
#if PTG_DEBUG
        if(sky_list[i] >= lcounts[0] + lcounts[1])   // positions of this round's queue (hits + sky)
        {
            if(sc.debug) atomicAdd(sc.debug + kDebugList, 1u);
            continue;
        }
#endif
        PathRec p;
        Hit h;
        bool occluded;
        load_queued<true>(cur, tr, sky_list[i], p, h, occluded, !FEAT && round > 0);
#if PTG_DEBUG
        debug_check_round(sc, p.meta, round);
#endif
        shade_path<COUNT, 2, MathExactLds, FEAT>(sc, p, h, occluded, out, cnt, mp, feat);
    }
    if(COUNT) flush_counters(cnt, counters, 0);
}

// One work-item per (pixel, sample).  A wave holds 8 pixels x 8 consecutive
// samples (one motion-blur subframe): lanes 0-7 are samples j..j+7 of pixel 0,
// and so on.  Consecutive waves walk the sample groups of one pixel group, so
// the waves in flight on a CU trace nearby pixels through the same TLASes.
template<bool COUNT>
__global__ __launch_bounds__(kBlock) void k_trace(DevScene sc, PixelMap pm, uint32_t j0, uint32_t nj,
                                                  float4* __restrict__ out, unsigned long long* __restrict__ counters)
{
    uint32_t p, jj;
    chunk_coords(blockIdx.x * blockDim.x + threadIdx.x, nj, p, jj);
    Counters cnt;
    if(p < pm.npix && jj < nj)
    {
        uint32_t x, y;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if(pm.pixel(p, x, y))
        {
            const f3 c = path_trace_sample<COUNT>(sc, x, y, (int32_t)(j0 + jj), cnt);
            r = make_float4(c.x, c.y, c.z, 0.f);
        }
        out[size_t(jj) * pm.npix + p] = r;
    }
    if(COUNT) flush_counters(cnt, counters, (p < pm.npix && jj < nj) ? 1u : 0u);
}

// The fold's arithmetic, each operation one float32 rounding (k_accumulate,
// k_ad_fold, image_math.h's close_*, tp_blend and ad_noisy share it).
//
// A chunk's nj samples of queue pixel q (npix queue pixels) added, in sample
// order, to the running radiance sum and, with MOMENTS, to the luminance
// moments (s1, s2, n) of the finite ones.
template<bool MOMENTS>
__device__ __forceinline__ void fold_samples(const float4* samples, uint32_t npix, uint32_t q, uint32_t nj,
                                             float& ax, float& ay, float& az, float& s1, float& s2, uint32_t& n)
{
    for(uint32_t j = 0; j < nj; ++j)
    {
        const float4 s = ld_out(samples + size_t(j) * npix + q);
        ax = ax + s.x;
        ay = ay + s.y;
        az = az + s.z;
        if constexpr(MOMENTS)
            if(finite3(V3(s.x, s.y, s.z)))
            {
                const float L = lum709(s.x, s.y, s.z);
                s1 = s1 + L;
                s2 = s2 + L * L;
                ++n;
            }
    }
}

// acc[p] (+)= samples in index order; on the last chunk / spp and tonemap.
// MOMENTS (ptg_render_moments): in the same pass over the chunk, the first two
// luminance moments of the finite samples too; the radiance sum is the same
// operation for operation.  mom[p] = (s1, s2, n as bits, -) carries across
// chunks as acc does; on the last chunk out.moments[p] = (m1, m2, variance of
// the mean, n), normalised by n, written unconditionally.  Without MOMENTS
// neither mom nor out.moments is touched: both may be null.  A queue pixel
// outside the image (tile maps) closes to zeros.
template<bool MOMENTS>
__global__ __launch_bounds__(kBlock) void k_accumulate(PixelMap pm, uint32_t nj, const float4* __restrict__ samples,
                                                       float4* __restrict__ acc, float4* __restrict__ mom, int first,
                                                       int last, float spp, Planes out)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if(p >= pm.npix) return;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
    uint32_t n = 0;
    if(!first)
    {
        const float4 a = acc[p];
        ax = a.x; ay = a.y; az = a.z;
        if constexpr(MOMENTS)
        {
            const float4 m = mom[p];
            s1 = m.x; s2 = m.y; n = __float_as_uint(m.z);
        }
    }
    fold_samples<MOMENTS>(samples, pm.npix, p, nj, ax, ay, az, s1, s2, n);
    if(!last)
    {
        acc[p] = make_float4(ax, ay, az, 0.f);
        if constexpr(MOMENTS) mom[p] = make_float4(s1, s2, __uint_as_float(n), 0.f);
        return;
    }
    uint32_t x, y;
    const bool inside = pm.pixel(p, x, y);
    close_radiance(ax, ay, az, spp, inside, out, p);
    if constexpr(MOMENTS) close_moments(s1, s2, n, inside, out, p);
}

// The feature fold of a fused render (ptg_render_with_features), beside
// k_accumulate and under its first / last protocol: the chunk's per-sample
// features (shade_path's FEAT stores, laid out like the samples) added in
// sample order to eight running sums per pixel, which start from +0 and carry
// across chunks in facc ([0, npix) albedo + coverage, [npix, 2 npix) normal +
// depth); on the last chunk each sum / spp into out.albedo and
// out.normal_depth (both given).  Per component that is k_features'
// arithmetic, acc = acc + v then acc / spp, so the bits are its bits.  Every
// value is read once: non-temporal loads, as the radiance fold's.
__global__ __launch_bounds__(kBlock) void k_fold_features(PixelMap pm, uint32_t nj, const float4* __restrict__ albedo,
                                                          const float4* __restrict__ normal_depth,
                                                          float4* __restrict__ facc, int first, int last, float spp,
                                                          Planes out)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if(p >= pm.npix) return;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), n = a;
    if(!first)
    {
        a = facc[p];
        n = facc[pm.npix + p];
    }
    for(uint32_t j = 0; j < nj; ++j)
    {
        const float4 va = ld_out(albedo + size_t(j) * pm.npix + p);
        const float4 vn = ld_out(normal_depth + size_t(j) * pm.npix + p);
        a.x = a.x + va.x; a.y = a.y + va.y; a.z = a.z + va.z; a.w = a.w + va.w;
        n.x = n.x + vn.x; n.y = n.y + vn.y; n.z = n.z + vn.z; n.w = n.w + vn.w;
    }
    if(!last)
    {
        facc[p] = a;
        facc[pm.npix + p] = n;
        return;
    }
    uint32_t x, y;
    if(!pm.pixel(p, x, y)) return;   // as k_features: a pixel outside the image is not written
    close_feature(a, spp, out.albedo, p);
    close_feature(n, spp, out.normal_depth, p);
}

__global__ __launch_bounds__(kBlock) void k_sample_list(DevScene sc, uint32_t n, const uint2* __restrict__ xy,
                                                        const int32_t* __restrict__ js, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    Counters cnt;
    const f3 c = path_trace_sample<false>(sc, xy[i].x, xy[i].y, js[i], cnt);
    out[i] = make_float4(c.x, c.y, c.z, 0.f);
}

__global__ __launch_bounds__(kBlock) void k_rays(DevScene sc, uint32_t tlas_root, uint32_t n,
                                                 const float* __restrict__ rays, uint32_t* __restrict__ hits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    const float* r = rays + size_t(i) * 8;
    const f3 o = V3(r[0], r[1], r[2]), d = V3(r[3], r[4], r[5]);
    Counters cnt;
    Hit h, unused;
    trace<false, false>(sc, tlas_root, 0, o, d, r[6], r[7], h, cnt);
    const bool shadow = trace<true, false>(sc, tlas_root, 0, o, d, r[6], r[7], unused, cnt);
    uint32_t* w = hits + size_t(i) * 8;
    w[0] = __float_as_uint(h.bx);
    w[1] = __float_as_uint(h.by);
    w[2] = __float_as_uint(h.bz);
    w[3] = __float_as_uint(h.thit);
    w[4] = h.instance_id;
    w[5] = h.primitive_id;
    w[6] = h.back_face ? 1u : 0u;
    w[7] = shadow ? 1u : 0u;
}

__global__ void k_scatter_tiles(PixelMap pm, const uchar4* __restrict__ tiles, uchar4* __restrict__ image)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if(p >= pm.npix) return;
    uint32_t x, y;
    if(pm.pixel(p, x, y)) image[size_t(y) * pm.img_w + x] = tiles[p];
}

// The frame from the gathered tile packs of a `world`-rank shard (ptg.h, tile
// packs), in gather form: one work-item per image pixel, so consecutive lanes
// store consecutive addresses of every output and load runs of tw consecutive
// slots.  Tile t = rank t % world's tile t / world; the pixel's slot is the
// same in all five planes of that rank's pack.  Pure copies: 16-byte loads
// (4 for the bytes), non-temporal since every slot is read once.  The host
// checked that pack_tiles covers every rank's tiles, so slot < slots.  The
// rank's pack is carved by pack_planes, as the render that wrote it carved it
// (the packs are only read); a uchar4 pixel moves as one word.
__global__ __launch_bounds__(kBlock) void k_assemble_tile_packs(uint32_t img_w, uint32_t npix, uint32_t tw, uint32_t th,
                                                                uint32_t tiles_x, uint32_t world, uint32_t slots,
                                                                size_t pack_bytes, const uint8_t* __restrict__ packs,
                                                                Planes out)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if(p >= npix) return;
    const uint32_t x = p % img_w, y = p / img_w;
    const uint32_t tx = x / tw, ty = y / th;
    const uint32_t t = ty * tiles_x + tx;
    const uint32_t rank = t % world, k = t / world;
    const uint32_t slot = k * (tw * th) + (y - ty * th) * tw + (x - tx * tw);
    const Planes in = pack_planes(const_cast<uint8_t*>(packs) + size_t(rank) * pack_bytes, slots);
    if(out.accum) as_f4(out.accum)[p] = nt_load(as_f4(in.accum) + slot);
    if(out.moments) as_f4(out.moments)[p] = nt_load(as_f4(in.moments) + slot);
    if(out.albedo) as_f4(out.albedo)[p] = nt_load(as_f4(in.albedo) + slot);
    if(out.normal_depth) as_f4(out.normal_depth)[p] = nt_load(as_f4(in.normal_depth) + slot);
    if(out.bgra)
        reinterpret_cast<uint32_t*>(out.bgra)[p] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(in.bgra) + slot);
}

// ---- first-hit feature buffers (the a-trous denoiser over them: image_ops.hip) ----

// The first ray path_trace_pixel traces for (pixel, sample): camera_ray's
// origin and direction with tmin 0 and tmax MAX_RAY_DIST, and the subframe.
__global__ __launch_bounds__(kBlock) void k_camera_rays(DevScene sc, uint32_t n, const uint2* __restrict__ xy,
                                                        const int32_t* __restrict__ js, float* __restrict__ rays,
                                                        uint32_t* __restrict__ subframe)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    const uint8_t* sf = subframe_of(sc, js[i]);
    u4 seed;
    f3 o, d;
    camera_ray(sc, sf, xy[i].x, xy[i].y, js[i], seed, o, d);
    float* r = rays + size_t(i) * 8;
    r[0] = o.x; r[1] = o.y; r[2] = o.z;
    r[3] = d.x; r[4] = d.y; r[5] = d.z;
    r[6] = 0.0f; r[7] = MAX_RAY_DIST;
    subframe[i] = (uint32_t)(sf - sc.subframes) / SF_STRIDE;
}

// Feature pass.  A wave holds 8 pixels x 8 consecutive samples, as k_trace
// does (lanes 0-7 are samples jb..jb+7 of the wave's pixel 0, and so on), so
// its primary rays are neighbours in the image and in time; it walks the
// sample range in groups of 8.  After each group the 8 lanes of a pixel fold
// the group's 8 values into the pixel's sums in sample order (every lane of
// the pixel keeps the same sums), so each component is the float32 sum
// ((0 + s_j0) + s_j0+1) + ... whatever the lane mapping.
__global__ __launch_bounds__(kBlock) void k_features(DevScene sc, PixelMap pm, uint32_t j0, uint32_t j1, float spp,
                                                     float4* __restrict__ out_albedo,
                                                     float4* __restrict__ out_normal_depth)
{
    // the walk stacks: the wavefront walks' LDS windows (LdsStack), one 64-lane
    // x kCap table per wave, with the lane's spill area in sc.spill
    __shared__ uint2 windows[kBlock * LdsStack::kCap];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = lane & 7u;
    BlockWalker<RegCold, LdsStack> w;
    w.st.bind(windows, threadIdx.x >> 6, lane, sc.spill + (size_t(blockIdx.x) * blockDim.x + threadIdx.x) * sc.spill_stride);
    // persistent blocks: block b takes the 32-pixel groups b, b + gridDim.x, ...
    const uint32_t groups = (pm.npix + kBlock / 8u - 1u) / (kBlock / 8u);
    for(uint32_t pb = blockIdx.x; pb < groups; pb += gridDim.x)
    {
        const uint32_t p = pb * (kBlock / 8u) + (threadIdx.x >> 3);
        uint32_t x = 0, y = 0;
        const bool inside = p < pm.npix && pm.pixel(p, x, y);
        float acc[8];
#pragma unroll
        for(int c = 0; c < 8; ++c) acc[c] = 0.0f;
        for(uint32_t jb = j0; jb < j1; jb += 8u)
        {
            // miss: albedo (1,1,1), coverage 0, normal 0, depth 0
            float v[8] = {1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            const uint32_t j = jb + k;
            bool active = inside && j < j1;
            const uint8_t* sf = subframe_of(sc, (int32_t)(active ? j : j0));
            f3 o = V3(0, 0, 0), d = V3(0, 0, 1);
            Counters cnt;
            if(active)
            {
                uint32_t tc, to;
                tlas_of(sc, sf, tc, to);
                u4 seed;
                camera_ray(sc, sf, x, y, (int32_t)j, seed, o, d);
                w.init(tc, o, d, 0.0f, MAX_RAY_DIST);
            }
            // the wave walks in phases as k_wf_walk does: node steps for the lanes
            // not standing at a leaf, then one leaf phase for the lanes that are
            const bool traced = active;
            while(__any(active))
            {
#pragma unroll
                for(int u = 0; u < kWalkUnroll; ++u)
                    if(active && !w.at_leaf() && w.template node_step<false>(sc, cnt) != 0) active = false;
                if(active && w.wants_leaf() && w.template leaf_step<false, false>(sc, cnt) != 0) active = false;
            }
            if(traced)
            {
                const Hit h = w.result();
                if(!(h.thit < 0))
                {
                    const HitInfo hi = hit_info<false, 0>(sc, light_of(sf), o, d, h, cnt);
                    const f3 n = hi.tbn.r[2];   // tangent_space keeps its argument as the third row
                    v[0] = hi.albedo.x; v[1] = hi.albedo.y; v[2] = hi.albedo.z; v[3] = 1.0f;
                    v[4] = n.x; v[5] = n.y; v[6] = n.z; v[7] = hi.thit;
                }
            }
            const uint32_t group = j1 - jb < 8u ? j1 - jb : 8u;
            for(uint32_t s = 0; s < group; ++s)
            {
                const int src = (int)((lane & 56u) + s);
#pragma unroll
                for(int c = 0; c < 8; ++c) acc[c] = acc[c] + __shfl(v[c], src);
            }
        }
        if(inside && k == 0)
        {
            out_albedo[p] = make_float4(acc[0] / spp, acc[1] / spp, acc[2] / spp, acc[3] / spp);
            out_normal_depth[p] = make_float4(acc[4] / spp, acc[5] / spp, acc[6] / spp, acc[7] / spp);
        }
    }
}

// ---- adaptive sampling ----

// A pass of ptg_render_adaptive: the rectangle its pixel ids index, the pass's
// share of the frame's subframes, and the ids of the pixels it samples.
struct AdaptivePass {
    uint32_t x0, y0, w, h;          // rectangle: pixel id = row * w + column
    uint32_t passes, pass, m;       // the pass owns subframes pass, pass + passes, ...; m samples each
    const uint32_t* list;           // the active pixels' ids
    uint32_t npix;                  // their number: the queue pixels of the pass

    // queue pixel p -> image pixel; an id outside the rectangle is a dead lane
    __device__ __forceinline__ bool pixel(uint32_t p, uint32_t& x, uint32_t& y) const
    {
        const uint32_t pix = list[p];
        if(pix >= w * h) return false;
        x = x0 + pix % w;
        y = y0 + pix / w;
        return true;
    }
    // local sample index of the pass -> sample index of the frame
    __device__ __forceinline__ uint32_t sample(uint32_t jl) const { return ((jl / m) * passes + pass) * m + jl % m; }
};

// The stopping rule on a pixel's running sums (s1, s2, n as bits, -): fewer
// than 2 finite samples, or the variance of the mean above (threshold * (mean
// + floor))^2; a NaN on either side of the comparison is noisy.
__device__ __forceinline__ bool ad_noisy(float4 mom, float threshold, float luminance_floor)
{
    const uint32_t n = __float_as_uint(mom.z);
    if(n < 2u) return true;
    const float4 m = moments_of(mom.x, mom.y, n);
    const float tol = threshold * (m.x + luminance_floor);
    return !(m.z <= tol * tol);
}

// Select and compact, one work-item per rectangle pixel: the pixel is active
// if any pixel of its (2 dilate + 1)^2 window, clipped to the rectangle, is
// noisy.  Active ids are appended per block - a ballot per wave, one atomic
// per block - in pixel order inside the block, so a row's neighbours stay
// neighbours in the list (the walks' coherence rests on 8-pixel groups); the
// order of the blocks is whatever the atomics give, and no result depends on
// it.  ALL: every pixel is active and the list is the identity (no atomics;
// *count is not touched).
template<bool ALL>
__global__ __launch_bounds__(kBlock) void k_ad_select(uint32_t w, uint32_t h, uint32_t dilate, float threshold,
                                                      float luminance_floor, const float4* __restrict__ mom,
                                                      uint32_t* __restrict__ list, uint32_t* __restrict__ count)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t npix = w * h;
    if constexpr(ALL)
    {
        if(p < npix) list[p] = p;
        return;
    }
    bool active = false;
    if(p < npix)
    {
        const int32_t x = (int32_t)(p % w), y = (int32_t)(p / w), r = (int32_t)dilate;
        for(int32_t dy = -r; dy <= r; ++dy)
        {
            const int32_t qy = y + dy;
            if(qy < 0 || qy >= (int32_t)h) continue;
            for(int32_t dx = -r; dx <= r; ++dx)
            {
                const int32_t qx = x + dx;
                if(qx < 0 || qx >= (int32_t)w) continue;
                active = active || ad_noisy(mom[size_t(qy) * w + size_t(qx)], threshold, luminance_floor);
            }
        }
    }
    __shared__ uint32_t wave_count[kBlock / 64], block_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(active);
    if(lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if(threadIdx.x == 0)
    {
        uint32_t total = 0;
        for(uint32_t k = 0; k < kBlock / 64; ++k) total += wave_count[k];
        block_base = total ? atomicAdd(count, total) : 0u;
    }
    __syncthreads();
    if(!active) return;
    uint32_t pos = block_base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    for(uint32_t k = 0; k < wave; ++k) pos += wave_count[k];
    list[pos] = p;   // pos < the number of active pixels <= npix
}

// The fold over the list: position q adds its chunk samples, in local sample
// order, into the running sums of the pixel it names - k_accumulate<true>'s
// operations on acc[pixel] = (sum.xyz, samples taken as bits) and mom[pixel] =
// (s1, s2, n as bits, -), both zeroed before the first pass.  A pixel that is
// not on the list keeps its sums.
__global__ __launch_bounds__(kBlock) void k_ad_fold(AdaptivePass ad, uint32_t nj, const float4* __restrict__ samples,
                                                    float4* __restrict__ acc, float4* __restrict__ mom)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= ad.npix) return;
    const uint32_t pix = ad.list[q];
    if(pix >= ad.w * ad.h) return;
    const float4 a = acc[pix], mo = mom[pix];
    float ax = a.x, ay = a.y, az = a.z;
    float s1 = mo.x, s2 = mo.y;
    uint32_t n = __float_as_uint(mo.z);
    fold_samples<true>(samples, ad.npix, q, nj, ax, ay, az, s1, s2, n);
    acc[pix] = make_float4(ax, ay, az, __uint_as_float(__float_as_uint(a.w) + nj));
    mom[pix] = make_float4(s1, s2, __uint_as_float(n), 0.f);
}

// The deferred resolve, one work-item per rectangle pixel: running sums `s`
// (only read) closed into the planes of `out` as the folds' last chunk closes
// them (image_math.h's close_*), outside any fold.  Each output may be null,
// and the plane behind a null output is not loaded: s.mom and s.feat may then
// be null too.
// PER_PIXEL = false (ptg_accum_resolve): every sum / div, the caller's spp or
// the samples the state holds.
// PER_PIXEL = true (ptg_render_adaptive): the divisor is the pixel's own
// sample count, acc.w as bits (k_ad_fold), which also goes to out_samples
// where given; `div` is not read.
template<bool PER_PIXEL>
__global__ __launch_bounds__(kBlock) void k_resolve(uint32_t npix, Sums s, float div, Planes out,
                                                    uint32_t* __restrict__ out_samples)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if(p >= npix) return;
    if(PER_PIXEL || out.accum || out.bgra)
    {
        const float4 a = as_f4(s.acc)[p];
        if constexpr(PER_PIXEL)
        {
            const uint32_t ns = __float_as_uint(a.w);
            div = (float)ns;
            if(out_samples) out_samples[p] = ns;
        }
        close_radiance(a.x, a.y, a.z, div, true, out, p);
    }
    if(out.moments)
    {
        const float4 mo = as_f4(s.mom)[p];
        close_moments(mo.x, mo.y, __float_as_uint(mo.z), true, out, p);
    }
    if(out.albedo) close_feature(as_f4(s.feat)[p], div, out.albedo, p);
    if(out.normal_depth) close_feature(as_f4(s.feat)[npix + p], div, out.normal_depth, p);
}

// ---------------------------------------------------------- render driver --

int check_cfg(const ptg_context* ctx, const ptg_render_config* cfg, uint32_t sample_end)
{
    if(!cfg || cfg->width == 0 || cfg->height == 0 || cfg->samples_per_pixel == 0 || cfg->samples_per_motion_blur_step == 0)
        return fail(PTG_E_INVALID, "bad render config");
    if(!ctx->scene_ready || !ctx->frame_ready) return fail(PTG_E_INVALID, "scene/frame not uploaded");
    if(sample_end > 0)
    {
        const uint64_t need = (uint64_t(sample_end) - 1) / cfg->samples_per_motion_blur_step + 1;
        if(need > ctx->subframe_count)
            return fail(PTG_E_RANGE, "sample range needs " + std::to_string(need) + " subframes, frame has " +
                                         std::to_string(ctx->subframe_count));
    }
    if(uint64_t(cfg->width) * cfg->height > (1ull << 31)) return fail(PTG_E_RANGE, "image too large");
    return PTG_OK;
}

// Kernel kinds for timing and work counters.
// (work counters use the first K_KINDS; the sky and classify kernels are timed
// separately and count into K_SHADE)
enum Kind : int { K_MEGA = 0, K_EXTEND = 1, K_SHADOW = 2, K_SHADE = 3, K_CAMERA = 4, K_ACCUM = 5, K_KINDS = 6,
                  K_SKY = 6, K_CLASSIFY = 7 };
// counting builds' device counters: 8 per kernel kind, the walk statistics
// (kWalkWords each for the closest-hit and the any-hit walk), then the
// certified shading's redo tallies (kRedoWords, tally_redo)
constexpr int kCounterWords = K_KINDS * 8 + 2 * kWalkWords + kRedoWords;

int timed_begin(ptg_context* ctx, int kind, hipStream_t st = nullptr)
{
    if(!ctx->timing) return PTG_OK;
    if(ctx->ev_used == ctx->ev_start.size())
    {
        hipEvent_t a, b;
        PTG_HIP(hipEventCreate(&a));
        PTG_HIP(hipEventCreate(&b));
        ctx->ev_start.push_back(a);
        ctx->ev_stop.push_back(b);
        ctx->ev_kind.push_back(0);
    }
    ctx->ev_kind[ctx->ev_used] = kind;
    PTG_HIP(hipEventRecord(ctx->ev_start[ctx->ev_used], st ? st : ctx->stream));
    return PTG_OK;
}

int timed_end(ptg_context* ctx, hipStream_t st = nullptr)
{
    if(!ctx->timing) return PTG_OK;
    PTG_HIP(hipEventRecord(ctx->ev_stop[ctx->ev_used++], st ? st : ctx->stream));
    return PTG_OK;
}

// A launch of the render path: the kernel's counting instantiation in a
// counting render, the plain one otherwise.  Both take the same arguments (a
// plain render passes null counter pointers, RenderJob::cnt_for).
template<typename... P, typename... A>
void launch_counted(const ptg_context* ctx, hipStream_t st, dim3 grid, uint32_t lds, void (*counting)(P...),
                    void (*plain)(P...), const A&... args)
{
    void (*const kernel)(P...) = ctx->counting ? counting : plain;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, st, args...);
}

// One timed launch of `kind` (launch_counted between timed_begin and
// timed_end), its launch error checked.  A kernel without a counting
// instantiation is passed twice.
template<typename... P, typename... A>
int launch(ptg_context* ctx, int kind, hipStream_t st, dim3 grid, uint32_t lds, void (*counting)(P...), void (*plain)(P...),
           const A&... args)
{
    if(int r = timed_begin(ctx, kind, st)) return r;
    launch_counted(ctx, st, grid, lds, counting, plain, args...);
    PTG_HIP(hipGetLastError());
    return timed_end(ctx, st);
}

// A render call's fixed parts, shared by the steps render_map and
// render_adaptive are made of.
struct RenderJob {
    ptg_context* ctx;
    const ptg_render_config* cfg;
    PixelMap pm;                           // in a pass of render_adaptive only npix counts: the list's length
    uint32_t j0, j1;                       // the sample range
    // what the range's last fold closes (render_adaptive: its resolve); with
    // albedo and normal_depth (both or neither, wavefront only) the render is
    // a fused one: round 0 stores the first-hit features per sample and
    // fold_chunk folds them too
    Planes out;
    // the running sums the folds carry, and only those: mom where the fold
    // keeps the luminance moments, feat in a fused render.  The context's own
    // (acc, mom, feat_acc: render_map sets them once they are grown), or with
    // `carried` the caller's (ptg_accum_add): then no chunk is the first or the
    // last and nothing is closed
    Sums sums;
    bool carried = false;
    bool moments() const { return out.moments != nullptr || sums.mom != nullptr; }
    bool fused() const { return out.albedo != nullptr || sums.feat != nullptr; }
    const AdaptivePass* ad = nullptr;      // render_adaptive: the pass whose list the chunks are traced and folded over
    uint32_t pipelines = 1;                // chunk pipelines (slots) in use
    uint32_t chunk = 0;                    // samples per chunk
    size_t M = 0;                          // queue positions of a full chunk
    uint32_t rounds = 0;                   // bounce rounds
    bool overlap = false;                  // wavefront: shadow walk and sky on the slots' side streams
    DevScene sc;
    size_t spill_region = 0;               // walk stack spill entries per (slot, walk kind)
    unsigned long long* cnt = nullptr;     // counting renders: the device counters
    uint32_t prev_slot = 0xFFFFFFFFu;      // the slot of the last fold
    // slot k's per-sample feature arrays, each pm.npix * chunk entries
    FeatOut<true> feat_of(uint32_t k) const
    {
        float4* base = ctx->slot[k].feat.as<float4>();
        const size_t n = size_t(pm.npix) * chunk;
        return FeatOut<true>{base, base + n, uint32_t(n)};
    }
    SlotState st[kWfSlots];
    // where a slot's next wavefront chunk stands (trace_chunk_wavefront)
    struct Cursor {
        uint32_t parity = 0;               // the PathSoA half of its round 0
        uint32_t chunks = 0;               // chunks traced on the slot so far: chunk k counts in block k & 1
        bool camera_queued = false;        // its camera kernel was hoisted into the chunk before it
    } cursor[kWfSlots];
    bool first_camera_queued = false;      // ctx->ev_first_camera is recorded in this render

    unsigned long long* cnt_for(int kind) const { return cnt ? cnt + 8 * kind : nullptr; }
    unsigned long long* ws_for(bool any) const { return cnt ? cnt + 8 * K_KINDS + (any ? kWalkWords : 0) : nullptr; }
    unsigned long long* redo_tally() const { return cnt ? cnt + 8 * K_KINDS + 2 * kWalkWords : nullptr; }
    // walk stack spill areas: one per (chunk pipeline, walk kind), since up to
    // four walk launches run at once; stack_bound entries per walk lane
    DevScene walk_scene(uint32_t slot, int kind) const
    {
        DevScene w = sc;
        w.spill = ctx->spill.as<uint2>() + (2 * slot + uint32_t(kind)) * spill_region;
        return w;
    }
    size_t lanes(uint32_t nj) const { return size_t((pm.npix + 7) / 8) * ((nj + 7) / 8) * 64; }
};

// A chunk: samples [j, j + n) on chunk pipeline `slot`.
struct Piece { uint32_t j, n, slot; };

// Chunk sizing: equal chunks of whole motion-blur groups (multiples of 8
// samples), each at most `target` paths.  The megakernel's target is 1 GiB of
// per-sample results.  Wavefront chunks are as large as HBM allows, up to
// 2^chunk_log2 paths: every bounce round then launches over a long queue, so
// the walk and shade launches run at full occupancy with short tails.  The
// slots' buffers are then grown to that size and their state carved.  A fused
// render (RenderJob::fused) budgets 32 B more per path and grows the slots'
// feature buffers; every other render sizes its chunks without them.
int size_chunks(RenderJob& job, bool wf)
{
    ptg_context* ctx = job.ctx;
    const uint32_t pipelines = job.pipelines;
    size_t target = (size_t(1) << 30) / sizeof(float4);
    if(wf)
    {
        size_t free_b = 0, total_b = 0;
        PTG_HIP(hipMemGetInfo(&free_b, &total_b));
        // + the path's per-sample result and, in a fused render, its two feature records
        const size_t per_path = kStateBytesPerPath + sizeof(float4) + (job.fused() ? 2 * sizeof(float4) : 0);
        // a slot's share of HBM, but never more than what is actually free (other
        // tenants, torch's cache): buffers this context already holds count as free
        size_t held = 0;
        for(uint32_t k = 0; k < pipelines; ++k)
            held += ctx->slot[k].state.bytes + ctx->slot[k].samples.bytes + (job.fused() ? ctx->slot[k].feat.bytes : 0);
        const size_t share = total_b / 100 * (pipelines > 2 ? ctx->hbm_pct * 2 / pipelines : ctx->hbm_pct);
        const size_t avail = (free_b + held) / 100 * 85 / pipelines;
        target = std::max<size_t>(size_t(1) << 16, std::min(size_t(1) << ctx->chunk_log2, std::min(share, avail) / per_path));
    }
    const uint32_t span = job.j1 - job.j0;
    const uint32_t max_chunk = std::max<uint32_t>(8, uint32_t(std::min<size_t>(target / size_t(job.pm.npix), span)) & ~7u);
    uint32_t nchunks = (span + max_chunk - 1) / max_chunk;
    if(pipelines > 1 && span >= 16u)
        nchunks = (std::max(nchunks, pipelines) + pipelines - 1) / pipelines * pipelines;   // whole rounds over the slots
    job.chunk = std::min<uint32_t>(span, ((span + nchunks - 1) / nchunks + 7) & ~7u);
    job.M = job.lanes(job.chunk);
    if(job.M >= (1ull << 31)) return fail(PTG_E_RANGE, "chunk too large");
    // the slots' buffers for chunks of that size: the samples and, wavefront, the path state
    for(uint32_t k = 0; k < pipelines; ++k)
    {
        PTG_HIP(ctx->grow(ctx->slot[k].samples, size_t(job.pm.npix) * job.chunk * sizeof(float4)));
        if(job.fused()) PTG_HIP(ctx->grow(ctx->slot[k].feat, 2 * size_t(job.pm.npix) * job.chunk * sizeof(float4)));
        if(!wf) continue;
        PTG_HIP(ctx->grow(ctx->slot[k].state, slot_state_bytes(job.M, job.rounds)));
        if(!carve_slot_state(ctx->slot[k].state.as<char>(), job.M, job.rounds, job.st[k]))
            return fail(PTG_E_INVALID, "the slot state's fields do not add up to kStateBytesPerPath");
    }
    return PTG_OK;
}

// The chunk plan, in sample order (the order the chunks are folded): equal
// chunks dealt round-robin to the slots.
std::vector<Piece> plan_chunks(const RenderJob& job)
{
    std::vector<Piece> plan;
    for(uint32_t j = job.j0, k = 0; j < job.j1; j += job.chunk, ++k)
        plan.push_back({j, std::min(job.chunk, job.j1 - j), k % job.pipelines});
    return plan;
}

// One chunk of the megakernel: every path from camera to its last bounce in one launch.
int trace_chunk_megakernel(RenderJob& job, const Piece& pc)
{
    ptg_context* ctx = job.ctx;
    return launch(ctx, K_MEGA, ctx->main_of(pc.slot), dim3(grid_for(job.lanes(pc.n))), 0, k_trace<true>, k_trace<false>, job.sc,
                  job.pm, pc.j, pc.n, ctx->slot[pc.slot].samples.as<float4>(), job.cnt_for(K_MEGA));
}

// One chunk of the wavefront pipeline on its slot's streams: the camera
// kernel, then per bounce round the closest-hit walk, the shadow walk of the
// previous round's NEE rays, classify, shade and sky.  With job.ad (a pass of
// render_adaptive) the camera kernel runs over the pass's pixel list, pc.j
// counting the pass's local samples; everything after it is the same.
//
// The hoisted camera.  `next` is the slot's next chunk of this render (null:
// none).  With a side stream (concurrency >= 1) its camera kernel is queued
// here, on the side stream inside this chunk's last round, so it runs beside
// that round's walk, classify and shade and beside the other slot's kernels,
// instead of alone between two chunks where nothing else of the slot can run
// (profiles/r06c_timeline/: both slots' cameras met there twice a frame).
// What it writes, and why nothing still in use:
//   - the PathSoA half S[(p + rounds) & 1] (SlotState).  Its last readers are
//     round `rounds - 2`'s extend, shadow, shade (which reads `cur`) and sky.
//     That sky kernel is ahead of the camera on the side stream, and it was
//     queued behind an event recorded on main after that round's shade, so
//     the main stream's readers are done as well.  With rounds < 2 the last
//     readers are the same kernels of the slot's chunk before this one, and
//     the same argument holds with that chunk's sky kernel.  The last round's
//     shade writes no survivor into the half (shade_path retires every path
//     at round == max_bounces).
//   - the other counts block, zeroed first on the same stream.  Its last user
//     is the chunk before this one, whose last sky kernel is ahead on the
//     side stream, behind its last shade.
//   - nothing else: not the sample buffer, which this chunk's fold has yet to
//     read (dead lanes: shade_path), neither TraceOut set, no list.  Nor a
//     fused render's feature buffer (Slot::feat), for the same reason as the
//     samples: this chunk's round 0 wrote it and this chunk's fold
//     (k_fold_features) has yet to read it; the next chunk's features are
//     written by its own round 0 shade and sky, behind that fold in stream order.
// The side stream also waits here for what main has queued so far: in a
// render's first chunk with rounds < 2 nothing else orders it behind the
// caller's upload of the frame the camera reads.
// What reads the camera's output, the next chunk's round 0 on main, is behind
// this chunk's closing join of the side stream.  The hoist adds no event: the
// slot's two are each recorded and waited for in one step, record first (the
// two lambdas below), so no wait can meet an event that is recorded later in
// submission order, which HIP would take as satisfied (the first cameras'
// event: see where it is used).
// On the side stream it stands behind the last round's shadow walk and the
// event classify waits for, and ahead of that round's sky kernel (ahead of
// the shadow walk, classify and shade wait for it too: measured slower,
// DESIGN 4.16).  Timing knobs, the frames do not depend on them:
// PTG_HOIST_CAMERA = 0 keeps every camera in order on main,
// PTG_CAMERAS_IN_TURN = 0 starts a render's first cameras side by side (below).
#ifndef PTG_HOIST_CAMERA
#define PTG_HOIST_CAMERA 1
#endif
#ifndef PTG_CAMERAS_IN_TURN
#define PTG_CAMERAS_IN_TURN 1
#endif
int trace_chunk_wavefront(RenderJob& job, const Piece& pc, const Piece* next = nullptr)
{
    ptg_context* ctx = job.ctx;
    const AdaptivePass* ad = job.ad;
    ptg_context::Slot& sl = ctx->slot[pc.slot];
    const SlotState& t = job.st[pc.slot];
    RenderJob::Cursor& at = job.cursor[pc.slot];
    const DevScene& sc = job.sc;
    const DevScene sc_ext = job.walk_scene(pc.slot, 0), sc_sh = job.walk_scene(pc.slot, 1);
    const uint32_t rounds = job.rounds;
    const uint32_t p = at.parity;
    uint32_t* counts = t.counts[at.chunks & 1];
    const hipStream_t ms = ctx->main_of(pc.slot);
    // second stream: the previous round's sky kernel, then this round's
    // shadow walk (independent of the closest-hit walk it runs beside)
    const hipStream_t ss = job.overlap ? sl.side : ms;
    auto side_after_main = [&]() -> int {
        if(!job.overlap) return PTG_OK;
        PTG_HIP(hipEventRecord(sl.ev_main, ms));
        PTG_HIP(hipStreamWaitEvent(sl.side, sl.ev_main, 0));
        return PTG_OK;
    };
    auto main_after_side = [&]() -> int {
        if(!job.overlap) return PTG_OK;
        PTG_HIP(hipEventRecord(sl.ev_side, sl.side));
        PTG_HIP(hipStreamWaitEvent(ms, sl.ev_side, 0));
        return PTG_OK;
    };
    auto grid_of = [&](const Piece& c) {
        return dim3(std::max<uint32_t>(1, std::min<uint32_t>(ctx->persistent_blocks, grid_for(job.lanes(c.n)))));
    };
    // chunk c's camera on stream st: zeroes counts block `cb` and fills half `half`
    auto camera = [&](const Piece& c, hipStream_t st, uint32_t half, uint32_t* cb) -> int {
        const uint32_t M = uint32_t(job.lanes(c.n));
        PTG_HIP(hipMemsetAsync(cb, 0, kCountWords(rounds) * sizeof(uint32_t), st));
        return ad ? launch(ctx, K_CAMERA, st, grid_of(c), 0, k_wf_camera<true, AdaptivePass>, k_wf_camera<false, AdaptivePass>,
                           sc, *ad, c.j, c.n, M, t.S[half], cb, job.cnt_for(K_CAMERA))
                  : launch(ctx, K_CAMERA, st, grid_of(c), 0, k_wf_camera<true, PixelMap>, k_wf_camera<false, PixelMap>, sc,
                           job.pm, c.j, c.n, M, t.S[half], cb, job.cnt_for(K_CAMERA));
    };
    float4* out = sl.samples.as<float4>();
    const bool feat0 = job.fused();
    const FeatOut<true> feat = feat0 ? job.feat_of(pc.slot) : FeatOut<true>{nullptr, nullptr, 0u};
    const dim3 grid = grid_of(pc);
    if(!at.camera_queued)
    {
        // The first cameras of a render take turns (concurrency 2): side by
        // side they take twice as long and no walk can start before one is
        // done, so slot k's waits for slot k - 1's, and slot 0's round-0 walk
        // starts after one camera's time with slot 1's camera beside it.  The
        // chunk plan deals a render's first chunks to slots 0, 1, ... in that
        // order, so the event is recorded before it is waited for, and
        // recorded again behind the camera that waited.
        const bool in_turn = PTG_CAMERAS_IN_TURN && job.pipelines > 1 && at.chunks == 0 && !ad;
        if(in_turn && job.first_camera_queued) PTG_HIP(hipStreamWaitEvent(ms, ctx->ev_first_camera, 0));
        if(int e = camera(pc, ms, p, counts)) return e;
        if(in_turn)
        {
            PTG_HIP(hipEventRecord(ctx->ev_first_camera, ms));
            job.first_camera_queued = true;
        }
    }
    // the slot's next chunk: the half and the counts block this one leaves free
    const bool hoist = PTG_HOIST_CAMERA && next && job.overlap && !ad;
    at.parity = (p + rounds) & 1;
    at.chunks += 1;
    at.camera_queued = hoist;
    auto hoisted_camera = [&]() -> int { return camera(*next, sl.side, at.parity, t.counts[at.chunks & 1]); };
    for(uint32_t r = 0; r < rounds; ++r)
    {
        const PathSoA& cur = t.S[(p + r) & 1];
        const PathSoA& nxt = t.S[(p + r + 1) & 1];
        const bool last = r + 1 == rounds;
        const TraceOut& tr = t.trs[r & 1];
        uint32_t* nee_next = t.lists[(r + 1) & 1];
        uint32_t* shadow_next = t.trs[(r + 1) & 1].shadow;
        if(hoist && last)
            if(int e = side_after_main()) return e;   // before this round's walk is queued: the camera is not to wait for it
        if(int e = launch(ctx, K_EXTEND, ms, ctx->walk_grid[0], ctx->walk_lds[0], k_wf_walk<false, true>,
                          k_wf_walk<false, false>, sc_ext, cur, counts, r, nullptr, tr, ctx->walk_xcds[0],
                          job.cnt_for(K_EXTEND), job.ws_for(false)))
            return e;
        if(r > 0)
            if(int e = launch(ctx, K_SHADOW, ss, ctx->walk_grid[1], ctx->walk_lds[1], k_wf_walk<true, true>,
                              k_wf_walk<true, false>, sc_sh, cur, counts, r, t.lists[r & 1], tr, ctx->walk_xcds[1],
                              job.cnt_for(K_SHADOW), job.ws_for(true)))
                return e;
        uint32_t* lc = counts + 2 * (rounds + 2) + 2 * r;   // this round's hit / sky list lengths
        uint32_t* rc = counts + 4 * (rounds + 2) + 2 * r;   // this round's redo list lengths (hit, sky)
        // classify/shade need the shadow results, the lists the previous sky
        // kernel read, and the state set it read
        if(int e = main_after_side()) return e;
        // the slot's next camera, behind the event classify waits for: it runs
        // beside the rest of this round's walk, classify and shade, and only
        // this round's sky kernel and the fold wait for it
        if(hoist && last)
            if(int e = hoisted_camera()) return e;
        if(int e = launch(ctx, K_CLASSIFY, ms, grid, 0, k_wf_classify, k_wf_classify, counts, r, tr, t.hit_list, t.sky_list, lc))
            return e;
        // the certified pass, then the exact pass over the paths it listed: one timed interval
        if(int e = timed_begin(ctx, K_SHADE, ms)) return e;
        // round 0 of a fused render: the instantiations that store the first-hit features too
        if(feat0 && r == 0)
            launch_counted(ctx, ms, grid, 0, k_wf_shade<true, ShadeMath, true>, k_wf_shade<false, ShadeMath, true>, sc, cur, nxt,
                           counts, r, tr, t.hit_list, lc, nee_next, shadow_next, out, t.redo_hit, rc, job.cnt_for(K_SHADE),
                           job.redo_tally(), feat);
        else
            launch_counted(ctx, ms, grid, 0, k_wf_shade<true, ShadeMath>, k_wf_shade<false, ShadeMath>, sc, cur, nxt, counts, r,
                           tr, t.hit_list, lc, nee_next, shadow_next, out, t.redo_hit, rc, job.cnt_for(K_SHADE),
                           job.redo_tally(), FeatOut<false>{});
        if constexpr(ShadeMath::kFast)
            launch_counted(ctx, ms, dim3(kRedoGrid), 0, k_wf_shade<true, MathExact>, k_wf_shade<false, MathExact>, sc, cur, nxt,
                           counts, r, tr, t.redo_hit, rc, nee_next, shadow_next, out, nullptr, nullptr, job.cnt_for(K_SHADE),
                           nullptr, FeatOut<false>{});
        PTG_HIP(hipGetLastError());
        if(int e = timed_end(ctx, ms)) return e;
        // escaped rays retire without feeding the next round: their
        // double-precision atmosphere runs on the second stream, overlapping
        // the next round's latency-bound walks (started beside shade instead,
        // the two compete for registers: 9% slower on frame 0)
        if(int e = side_after_main()) return e;
        if(int e = feat0 && r == 0 ? launch(ctx, K_SKY, ss, grid, 0, k_wf_sky<true, true>, k_wf_sky<false, true>, sc, cur, tr, r,
                                            t.sky_list, lc, out, job.cnt_for(K_SHADE), feat)
                                   : launch(ctx, K_SKY, ss, grid, 0, k_wf_sky<true>, k_wf_sky<false>, sc, cur, tr, r, t.sky_list,
                                            lc, out, job.cnt_for(K_SHADE), FeatOut<false>{}))
            return e;
    }
    return main_after_side();   // join before the fold
}

// The fold of a chunk (k_accumulate: its samples into the running per-pixel
// sums, chunks in sample order) runs on the chunk's own slot stream right
// after the chunk; a fold whose predecessor ran on the other slot first
// waits for that fold's event.  (A separate accumulation stream shared a
// hardware queue with slot 0's stream - HIP maps five streams onto
// GPU_MAX_HW_QUEUES = 4 queues - so a fold waiting for slot 1's chunk
// blocked slot 0's next launches behind it: profiles/r06c_timeline/.)
// A slot's next chunk then reuses its samples buffer after its fold in
// stream order, with no event at all.  A render that keeps the samples'
// moments (ptg_render_moments) folds with k_accumulate<true>, in the same
// place and order; k_accumulate<false> touches neither the moment sums nor
// out.moments (both null then).  The sums are job.sums, whoever owns them.
// A fused render (ptg_render_with_features) folds the
// chunk's features with k_fold_features right behind it, ahead of the event:
// the feature sums follow the same chain.  A pass of render_adaptive folds
// with k_ad_fold over its list; job.prev_slot runs through the whole render,
// so a pass's first fold follows the last fold of the pass before it.
int fold_chunk(RenderJob& job, const Piece& pc)
{
    ptg_context* ctx = job.ctx;
    ptg_context::Slot& sl = ctx->slot[pc.slot];
    // ptg_accum_add (job.carried): the sums are the caller's planes and no chunk
    // is the first or the last - the fold reads them, adds and writes them back
    // (a zeroed plane starts from +0 as `first` does), and divides nothing
    const int first = !job.carried && pc.j == job.j0, last = !job.carried && pc.j + pc.n >= job.j1;
    float4 *const acc = as_f4(job.sums.acc), *const mom = as_f4(job.sums.mom);
    const hipStream_t as = ctx->main_of(pc.slot);
    if(job.pipelines > 1 && job.prev_slot != 0xFFFFFFFFu && job.prev_slot != pc.slot)
        PTG_HIP(hipStreamWaitEvent(as, ctx->slot[job.prev_slot].ev_acc, 0));
    const auto fold = job.moments() ? k_accumulate<true> : k_accumulate<false>;
    const dim3 grid(grid_for(job.pm.npix));
    if(int r = job.ad ? launch(ctx, K_ACCUM, as, grid, 0, k_ad_fold, k_ad_fold, *job.ad, pc.n, sl.samples.as<float4>(), acc, mom)
                      : launch(ctx, K_ACCUM, as, grid, 0, fold, fold, job.pm, pc.n, sl.samples.as<float4>(), acc, mom, first,
                               last, (float)job.cfg->samples_per_pixel, job.out))
        return r;
    if(job.fused())
    {   // the features of the chunk, directly behind its samples: same stream, same order, same event
        const FeatOut<true> f = job.feat_of(pc.slot);
        if(int r = launch(ctx, K_ACCUM, as, grid, 0, k_fold_features, k_fold_features, job.pm, pc.n, f.albedo, f.normal_depth,
                          as_f4(job.sums.feat), first, last, (float)job.cfg->samples_per_pixel, job.out))
            return r;
    }
    if(job.pipelines > 1) PTG_HIP(hipEventRecord(sl.ev_acc, as));
    job.prev_slot = pc.slot;
    return PTG_OK;
}

#if PTG_DEBUG
// PTG_DEBUG builds: the render's violation tallies, layout.h's kDebug* slots (waits for the render)
int check_debug_tallies(ptg_context* ctx)
{
    uint32_t dbg[kDebugSlots];
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    PTG_HIP(hipMemcpy(dbg, ctx->debug.p, sizeof(dbg), hipMemcpyDeviceToHost));
    std::string bad;
    static const char* names[kDebugSlots] = {"node record", "triangle", "instance", "NEE list", "shade list", "walk stack", "", ""};
    for(uint32_t k = 0; k < kDebugSlots; ++k)
        if(dbg[k])
            bad += std::string(bad.empty() ? "" : ", ") +
                   (k == kDebugRound ? std::string("path state of another round loaded") : std::string(names[k]) + " index out of range") +
                   " x" + std::to_string(dbg[k]);
    if(bad.empty()) return PTG_OK;
    PTG_HIP(hipMemset(ctx->debug.p, 0, sizeof(dbg)));
    return fail(PTG_E_RANGE, "PTG_DEBUG: " + bad);
}
#endif

// Counting renders: the device counters into the context (waits for the render).
int read_counters(ptg_context* ctx)
{
    unsigned long long host[kCounterWords];
    PTG_HIP(hipMemcpyAsync(host, ctx->counters.p, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    for(int w = 0; w < 2; ++w)   // (the WalkExtra words behind them are ptg_walk_rays' alone)
        for(int k = 0; k < WS_COUNT; ++k) ctx->walk_stats[w][k] = host[K_KINDS * 8 + w * kWalkWords + k];
    for(int k = 0; k < kRedoWords; ++k) ctx->redo_stats[k] = host[K_KINDS * 8 + 2 * kWalkWords + k];
    for(int i = 0; i < 8; ++i)
    {
        ctx->last_counters[i] = 0;
        for(int k = 0; k < K_KINDS; ++k)
        {
            ctx->kind_counters[k][i] = host[k * 8 + i];
            ctx->last_counters[i] += host[k * 8 + i];
        }
    }
    return PTG_OK;
}

// A render's ending: a PTG_DEBUG build's tallies, a counting render's counters.
int end_render(ptg_context* ctx)
{
#if PTG_DEBUG
    if(int r = check_debug_tallies(ctx)) return r;
#endif
    return ctx->counting ? read_counters(ctx) : PTG_OK;
}

// A render's fixed setup: the chunk pipelines in use, the bounce rounds, a
// counting render's counters (zeroed on the caller's stream), the scene
// arguments and the walks' spill areas.
int begin_render(RenderJob& job, bool wf)
{
    ptg_context* ctx = job.ctx;
    job.pipelines = (wf && ctx->concurrency >= 2) ? kWfSlots : 1u;
    job.rounds = job.cfg->max_bounces + 1;
    job.overlap = wf && ctx->concurrency >= 1;
    if(ctx->counting)
    {
        PTG_HIP(ctx->grow(ctx->counters, kCounterWords * sizeof(unsigned long long)));
        PTG_HIP(hipMemsetAsync(ctx->counters.p, 0, kCounterWords * sizeof(unsigned long long), ctx->stream));
        job.cnt = ctx->counters.as<unsigned long long>();
    }
    job.sc = ctx->scene_args(job.cfg);
    job.spill_region = size_t(std::max(ctx->walk_grid[0], ctx->walk_grid[1])) * kBlock * ctx->stack_bound;
    if(wf) PTG_HIP(ctx->grow(ctx->spill, std::max<size_t>(1, 2 * job.pipelines * job.spill_region) * sizeof(uint2)));
    return PTG_OK;
}

// The other slots start after what the caller's stream holds so far: the
// caller's own work, the zeroed counters and whatever else the render queued
// there before its first chunk.
int start_slots(const RenderJob& job)
{
    ptg_context* ctx = job.ctx;
    if(job.pipelines < 2) return PTG_OK;
    PTG_HIP(hipEventRecord(ctx->ev_render_start, ctx->stream));
    for(uint32_t k = 1; k < job.pipelines; ++k)
        PTG_HIP(hipStreamWaitEvent(ctx->slot[k].main, ctx->ev_render_start, 0));
    return PTG_OK;
}

// The caller's stream after the render's last fold so far: it sees every chunk folded.
int join_folds(const RenderJob& job)
{
    if(job.pipelines > 1 && job.prev_slot != 0xFFFFFFFFu && job.prev_slot != 0)
        PTG_HIP(hipStreamWaitEvent(job.ctx->stream, job.ctx->slot[job.prev_slot].ev_acc, 0));
    return PTG_OK;
}

// Render the pixels of `pm` for samples [j0, j1) into the planes of `out`: per
// chunk of samples, the path kernels write one float4 per (pixel, sample);
// k_accumulate folds the chunk into the running per-pixel sum in sample order,
// with out.moments the luminance moments too.
// With out.albedo and out.normal_depth (both; wavefront only: render_planes)
// round 0 also stores every sample's first-hit features and k_fold_features
// folds them.
// With `carried` (ptg_accum_add; `out` empty) the chunks fold into the
// caller's sums, moments and features as the sums say, and nothing is
// closed: the context's own sums are not touched.
int render_map(ptg_context* ctx, const ptg_render_config* cfg, PixelMap pm, uint32_t j0, uint32_t j1, const Planes& out,
               const Sums* carried = nullptr)
{
    if(pm.npix == 0) return PTG_OK;
    if(j1 <= j0) return fail(PTG_E_INVALID, "empty sample range");
    const bool wf = ctx->pipeline == 0;
    if(!wf && ctx->stack_bound >= PrivStack::kCap)
        return fail(PTG_E_RANGE, "the megakernel's walk stack holds " + std::to_string(PrivStack::kCap) +
                                     " entries, this frame's BVHs need " + std::to_string(ctx->stack_bound));
    RenderJob job{ctx, cfg, pm, j0, j1, out};
    if(carried)
    {
        job.sums = *carried;
        job.carried = true;
    }
    if(job.fused() && !wf) return fail(PTG_E_INVALID, "render_map: fused features run on the wavefront pipeline");
    if(int r = begin_render(job, wf)) return r;
    if(int r = size_chunks(job, wf)) return r;
    if(!carried)
    {   // the context's own sums, grown to the map
        PTG_HIP(ctx->grow(ctx->acc, size_t(pm.npix) * sizeof(float4)));
        job.sums.acc = ctx->acc.as<ptg_float4>();
        if(job.fused())
        {
            PTG_HIP(ctx->grow(ctx->feat_acc, 2 * size_t(pm.npix) * sizeof(float4)));
            job.sums.feat = ctx->feat_acc.as<ptg_float4>();
        }
        if(out.moments)
        {
            PTG_HIP(ctx->grow(ctx->mom, size_t(pm.npix) * sizeof(float4)));
            job.sums.mom = ctx->mom.as<ptg_float4>();
        }
    }
    if(int r = start_slots(job)) return r;
    const std::vector<Piece> plan = plan_chunks(job);
    for(size_t k = 0; k < plan.size(); ++k)
    {
        const Piece& pc = plan[k];
        const Piece* next = k + job.pipelines < plan.size() ? &plan[k + job.pipelines] : nullptr;   // the slot's next chunk
        if(int r = wf ? trace_chunk_wavefront(job, pc, next) : trace_chunk_megakernel(job, pc)) return r;
        if(int r = fold_chunk(job, pc)) return r;
    }
    if(int r = join_folds(job)) return r;
    return end_render(ctx);
}

// ptg_render_adaptive once its arguments are checked (wavefront pipeline):
// render_map's chunk pipelines, slots and event scheme over `passes` passes of
// N / passes samples each.  A pass traces and folds the pixels of the list in
// ctx->ad_list (job.ad; size_chunks / plan_chunks with npix = the list's
// length); after a pass from min_passes on, k_ad_select rebuilds the list from
// the running sums and the host reads its length - the render's only wait.
// The running sums (job.sums) are ctx->acc and ctx->mom, indexed by rectangle
// pixel; k_resolve<true> closes them into `out` and out_samples.
int render_adaptive(ptg_context* ctx, const ptg_render_config* cfg, const PixelMap& rect, const ptg_adaptive_params& P,
                    const Planes& out, uint32_t* out_samples)
{
    ctx->ad_passes_run = 0;
    for(uint64_t& a: ctx->ad_active) a = 0;
    const uint32_t npix = rect.npix;
    if(npix == 0) return PTG_OK;
    RenderJob job{ctx, cfg, rect, 0, cfg->samples_per_pixel / P.passes, out};
    PTG_HIP(ctx->grow(ctx->acc, size_t(npix) * sizeof(float4)));
    PTG_HIP(ctx->grow(ctx->mom, size_t(npix) * sizeof(float4)));
    PTG_HIP(ctx->grow(ctx->ad_list, size_t(npix) * sizeof(uint32_t)));
    PTG_HIP(ctx->grow(ctx->ad_count, 256));
    uint32_t* list = ctx->ad_list.as<uint32_t>();
    uint32_t* count = ctx->ad_count.as<uint32_t>();
    job.sums = Sums{ctx->acc.as<ptg_float4>(), ctx->mom.as<ptg_float4>()};
    float4 *const acc = as_f4(job.sums.acc), *const mom = as_f4(job.sums.mom);
    if(int r = begin_render(job, true)) return r;
    // the sums start from +0; before min_passes every pixel is active.  The
    // other slots start behind the zeroed sums and the first list.
    PTG_HIP(hipMemsetAsync(acc, 0, size_t(npix) * sizeof(float4), ctx->stream));
    PTG_HIP(hipMemsetAsync(mom, 0, size_t(npix) * sizeof(float4), ctx->stream));
    if(int r = launch_plain(ctx, grid_for(npix), k_ad_select<true>, rect.w, rect.h, 0u, 0.0f, 0.0f, mom, list, count)) return r;
    if(int r = start_slots(job)) return r;
    uint32_t len = npix;
    AdaptivePass ad{rect.x0, rect.y0, rect.w, rect.h, P.passes, 0, cfg->samples_per_motion_blur_step, list, len};
    job.ad = &ad;
    for(uint32_t k = 0; k < P.passes && len > 0; ++k)
    {
        ctx->ad_active[k] = len;
        ctx->ad_passes_run = k + 1;
        ad.pass = k;
        ad.npix = job.pm.npix = len;
        if(int r = size_chunks(job, true)) return r;
        for(const Piece& pc: plan_chunks(job))
        {
            if(int r = trace_chunk_wavefront(job, pc)) return r;
            if(int r = fold_chunk(job, pc)) return r;
        }
        if(k + 1 < P.min_passes || k + 1 >= P.passes) continue;
        // selection: every pixel of the rectangle on its current sums
        if(int r = join_folds(job)) return r;
        PTG_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), ctx->stream));
        if(int r = launch_plain(ctx, grid_for(npix), k_ad_select<false>, rect.w, rect.h, P.dilate, P.threshold,
                                P.luminance_floor, mom, list, count))
            return r;
        PTG_HIP(hipMemcpyAsync(&len, count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        PTG_HIP(hipStreamSynchronize(ctx->stream));
        if(len > npix) return fail(PTG_E_RANGE, "ptg_render_adaptive: the active list is longer than the rectangle");
    }
    if(int r = join_folds(job)) return r;
    if(int r = launch_plain(ctx, grid_for(npix), k_resolve<true>, npix, job.sums, 0.0f, out, out_samples)) return r;
    return end_render(ctx);
}

} // namespace

extern "C" {

// a launch-geometry knob from the environment (timing experiments only:
// no result depends on it), else its default
static uint32_t env_knob(const char* name, uint32_t dflt)
{
    const char* v = getenv(name);
    if(!v || !*v) return dflt;
    char* end = nullptr;
    const unsigned long x = strtoul(v, &end, 10);
    return (end && *end == 0 && x <= 64) ? uint32_t(x) : dflt;
}

int ptg_context_create(int device, ptg_context** out)
{
    if(!out) return fail(PTG_E_INVALID, "null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if(e != hipSuccess || n == 0) return fail(PTG_E_NODEVICE, "no HIP device available");
    if(device < 0 || device >= n) return fail(PTG_E_NODEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    PTG_HIP(hipGetDeviceProperties(&prop, device));
    if(strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PTG_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950");
    std::unique_ptr<ptg_context> ctx(new ptg_context());
    ctx->device = device;
    // grid-stride kernels (camera, classify, shade, sky): 32 blocks per CU,
    // measured best of 3..128
    ctx->persistent_blocks = uint32_t(std::max(1, prop.multiProcessorCount)) * 32u;
    // timing knobs: chunk size and HBM share of a renderer that owns the GPU
    ctx->chunk_log2 = std::min<uint32_t>(28u, std::max<uint32_t>(16u, env_knob("PTG_CHUNK_LOG2", ctx->chunk_log2)));
    ctx->hbm_pct = std::min<uint32_t>(70u, std::max<uint32_t>(5u, env_knob("PTG_HBM_SHARE", ctx->hbm_pct)));
    // Walk residency: each walk lane holds its world ray (32 B) and its stack
    // window (8 x kCap B) in LDS, so the walk blocks' LDS sets how many are
    // resident per CU: kWalkResident (the LDS is padded to that share).
    const uint32_t lds_cu = prop.maxSharedMemoryPerMultiProcessor ? uint32_t(prop.maxSharedMemoryPerMultiProcessor) : 65536u;
    const uint32_t lds_need[2] = {kBlock * uint32_t(sizeof(WalkCold) + WalkStackOf<false>::type::kLaneBytes),
                                  kBlock * uint32_t(sizeof(WalkCold) + WalkStackOf<true>::type::kLaneBytes)};
    for(int k = 0; k < 2; ++k)
    {
        const uint32_t resident = env_knob(k ? "PTG_WALK_RESIDENT_ANY" : "PTG_WALK_RESIDENT", kWalkResident[k]);
        ctx->walk_lds[k] = std::max<uint32_t>(lds_need[k], resident ? (lds_cu / resident) / 1024u * 1024u : 0u);
    }
    // One wave of walk blocks, 3 per CU although the LDS holds 4: every block
    // is resident from the start (no oversubscription), and the fourth slot's
    // LDS and registers take the other chunk pipeline's shade and sky waves,
    // which cannot sit beside four walk blocks (their LDS fills the CU).
    // Measured at 1024 spp against the round-1 choice (4 x the resident grid):
    // frame 0 464 vs 495 ms, frame 450 2827 vs 2843, frame 1400 2004 vs 2012
    // (profiles/r02o_grid/).
    int per_cu = 0;
    const void* walks[2] = {reinterpret_cast<const void*>(k_wf_walk<false, false>),
                            reinterpret_cast<const void*>(k_wf_walk<true, false>)};
    for(int k = 0; k < 2; ++k)
    {
        per_cu = 0;
        if(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, walks[k], kBlock, ctx->walk_lds[k]) != hipSuccess ||
           per_cu <= 0)
            per_cu = int(kWalkResident[k] ? kWalkResident[k] : 1u);
        const uint32_t blocks = env_knob(k ? "PTG_WALK_BLOCKS_ANY" : "PTG_WALK_BLOCKS", kWalkBlocksPerCu[k]);
        ctx->walk_grid[k] = std::min<uint32_t>(uint32_t(per_cu), std::max(1u, blocks)) * uint32_t(prop.multiProcessorCount);
        ctx->walk_xcds[k] = (ctx->walk_grid[k] % 8 == 0 && kBands % 8 == 0) ? 8u : 1u;
    }
    PTG_HIP(hipSetDevice(device));
#if PTG_DEBUG
    PTG_HIP(ctx->debug.reserve(kDebugSlots * sizeof(uint32_t)));
    PTG_HIP(hipMemset(ctx->debug.p, 0, kDebugSlots * sizeof(uint32_t)));
#endif
    for(uint32_t k = 0; k < kWfSlots; ++k)
    {
        ptg_context::Slot& b = ctx->slot[k];
        if(k > 0) PTG_HIP(hipStreamCreateWithFlags(&b.main, hipStreamNonBlocking));   // slot 0: the caller's stream
        PTG_HIP(hipStreamCreateWithFlags(&b.side, hipStreamNonBlocking));
        for(hipEvent_t* e: {&b.ev_main, &b.ev_side, &b.ev_acc})
            PTG_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    PTG_HIP(hipEventCreateWithFlags(&ctx->ev_render_start, hipEventDisableTiming));
    PTG_HIP(hipEventCreateWithFlags(&ctx->ev_first_camera, hipEventDisableTiming));
    *out = ctx.release();
    return PTG_OK;
}

void ptg_context_destroy(ptg_context* ctx)
{
    if(!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    delete ctx;
}

int ptg_context_get_stream(ptg_context* ctx, void** out)
{
    if(!ctx || !out) return fail(PTG_E_INVALID, "ptg_context_get_stream: null argument");
    *out = static_cast<void*>(ctx->stream);
    return PTG_OK;
}

int ptg_context_device(ptg_context* ctx, int* out)
{
    if(!ctx || !out) return fail(PTG_E_INVALID, "ptg_context_device: null argument");
    *out = ctx->device;
    return PTG_OK;
}

int ptg_context_set_stream(ptg_context* ctx, void* stream)
{
    if(int r = bind(ctx)) return r;
    hipStream_t next = static_cast<hipStream_t>(stream);
    if(next != ctx->stream)
    {   // work queued on the old stream (a render still reading blocks,
        // inst_trav, tlas_root) comes before anything queued on the new one,
        // e.g. the next frame's upload
        hipEvent_t ev;
        PTG_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, ctx->stream);
        if(e == hipSuccess) e = hipStreamWaitEvent(next, ev, 0);
        (void)hipEventDestroy(ev);
        if(e != hipSuccess) return hip_fail(e, "ptg_context_set_stream: ordering the old stream before the new");
    }
    ctx->stream = next;
    return PTG_OK;
}

static int rect_map(const ptg_render_config* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, PixelMap& pm)
{
    if(uint64_t(x0) + w > cfg->width || uint64_t(y0) + h > cfg->height) return fail(PTG_E_RANGE, "rectangle outside the image");
    pm = PixelMap{};
    pm.tiles = 0;
    pm.x0 = x0; pm.y0 = y0; pm.w = w; pm.h = h;
    pm.img_w = cfg->width; pm.img_h = cfg->height;
    pm.npix = w * h;
    return PTG_OK;
}

int ptg_render(ptg_context* ctx, const ptg_render_config* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
               uint32_t sample_begin, uint32_t sample_end, ptg_float4* out_accum, ptg_uchar4* out_bgra)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, sample_end)) return r;
    PixelMap pm;
    if(int r = rect_map(cfg, x0, y0, w, h, pm)) return r;
    return render_map(ctx, cfg, pm, sample_begin, sample_end, Planes{out_accum, out_bgra});
}

int ptg_render_moments(ptg_context* ctx, const ptg_render_config* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                       uint32_t sample_begin, uint32_t sample_end, ptg_float4* out_accum, ptg_uchar4* out_bgra,
                       ptg_float4* out_moments)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, sample_end)) return r;
    if(!out_moments) return fail(PTG_E_INVALID, "ptg_render_moments: null out_moments");
    PixelMap pm;
    if(int r = rect_map(cfg, x0, y0, w, h, pm)) return r;
    return render_map(ctx, cfg, pm, sample_begin, sample_end, Planes{out_accum, out_bgra, out_moments});
}

void ptg_adaptive_params_default(ptg_adaptive_params* p)
{
    if(!p) return;
    // the best row of tools/denoise_study.py --adaptive --sweep (profiles/denoise_study/adaptive_study.json)
    p->passes = 8;
    p->min_passes = 1;
    p->dilate = 2;
    p->threshold = 0.025f;
    p->luminance_floor = 0.01f;
}

int ptg_render_adaptive(ptg_context* ctx, const ptg_render_config* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                        const ptg_adaptive_params* params, ptg_float4* out_accum, ptg_uchar4* out_bgra,
                        ptg_float4* out_moments, uint32_t* out_samples)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, cfg ? cfg->samples_per_pixel : 0)) return r;
    if(!params) return fail(PTG_E_INVALID, "ptg_render_adaptive: null params");
    const ptg_adaptive_params P = *params;
    if(P.min_passes < 1 || P.min_passes > P.passes || P.passes > 16)
        return fail(PTG_E_INVALID, "ptg_render_adaptive: 1 <= min_passes <= passes <= 16");
    if(P.dilate > 2) return fail(PTG_E_INVALID, "ptg_render_adaptive: dilate is 0, 1 or 2");
    for(float s: {P.threshold, P.luminance_floor})
        if(!(s > 0.0f) || !std::isfinite(s))
            return fail(PTG_E_INVALID, "ptg_render_adaptive: threshold and luminance_floor must be positive and finite");
    if(uint64_t(cfg->samples_per_pixel) % (uint64_t(P.passes) * cfg->samples_per_motion_blur_step))
        return fail(PTG_E_INVALID, "ptg_render_adaptive: samples_per_pixel must be a multiple of passes * samples_per_motion_blur_step");
    if(!out_accum && !out_bgra && !out_moments && !out_samples) return fail(PTG_E_INVALID, "ptg_render_adaptive: no output given");
    if(ctx->pipeline != 0)
        return fail(PTG_E_INVALID, "ptg_render_adaptive: runs on the wavefront pipeline only (ptg_set_pipeline(ctx, 0))");
    PixelMap pm;
    if(int r = rect_map(cfg, x0, y0, w, h, pm)) return r;
    return render_adaptive(ctx, cfg, pm, P, Planes{out_accum, out_bgra, out_moments}, out_samples);
}

int ptg_last_adaptive_stats(ptg_context* ctx, uint32_t* passes_run, uint64_t active[16])
{
    if(!ctx || !passes_run || !active) return fail(PTG_E_INVALID, "ptg_last_adaptive_stats: bad arguments");
    *passes_run = ctx->ad_passes_run;
    memcpy(active, ctx->ad_active, sizeof(ctx->ad_active));
    return PTG_OK;
}

static int tile_map(const ptg_render_config* cfg, uint32_t tw, uint32_t th, uint32_t first, uint32_t stride,
                    uint32_t count, PixelMap& pm)
{
    if(tw == 0 || th == 0 || stride == 0) return fail(PTG_E_INVALID, "bad tile geometry");
    const uint32_t tx = (cfg->width + tw - 1) / tw, ty = (cfg->height + th - 1) / th;
    if(count && uint64_t(first) + uint64_t(count - 1) * stride >= uint64_t(tx) * ty)
        return fail(PTG_E_RANGE, "tile index beyond the image");
    if(uint64_t(count) * tw * th >= (1ull << 31)) return fail(PTG_E_RANGE, "too many tile pixels");
    pm = PixelMap{};
    pm.tiles = 1;
    pm.tw = tw; pm.th = th; pm.tiles_x = tx; pm.first = first; pm.stride = stride;
    pm.img_w = cfg->width; pm.img_h = cfg->height;
    pm.npix = count * tw * th;
    return PTG_OK;
}

int ptg_render_tiles(ptg_context* ctx, const ptg_render_config* cfg, uint32_t tile_w, uint32_t tile_h, uint32_t first_tile,
                     uint32_t tile_stride, uint32_t tile_count, ptg_float4* out_accum, ptg_uchar4* out_bgra)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, cfg ? cfg->samples_per_pixel : 0)) return r;
    PixelMap pm;
    if(int r = tile_map(cfg, tile_w, tile_h, first_tile, tile_stride, tile_count, pm)) return r;
    return render_map(ctx, cfg, pm, 0, cfg->samples_per_pixel, Planes{out_accum, out_bgra});
}

int ptg_scatter_tiles(ptg_context* ctx, const ptg_render_config* cfg, uint32_t tile_w, uint32_t tile_h,
                      uint32_t first_tile, uint32_t tile_stride, uint32_t tile_count, const ptg_uchar4* tiles,
                      ptg_uchar4* image)
{
    if(int r = bind(ctx)) return r;
    if(!cfg || !tiles || !image) return fail(PTG_E_INVALID, "ptg_scatter_tiles: bad arguments");
    PixelMap pm;
    if(int r = tile_map(cfg, tile_w, tile_h, first_tile, tile_stride, tile_count, pm)) return r;
    if(pm.npix == 0) return PTG_OK;
    return launch_plain(ctx, grid_for(pm.npix), k_scatter_tiles, pm, reinterpret_cast<const uchar4*>(tiles),
                        reinterpret_cast<uchar4*>(image));
}

// An explicit (pixel, sample) list: checked against the image and the frame's
// subframes, then copied to tmp_a (xy) and tmp_b (sample indices).
static int upload_sample_list(ptg_context* ctx, const ptg_render_config* cfg, size_t n, const ptg_uint2* xy,
                              const int32_t* sample_index)
{
    int32_t jmax = 0;
    for(size_t i = 0; i < n; ++i)
    {
        jmax = std::max(jmax, sample_index[i]);
        if(xy[i].x >= cfg->width || xy[i].y >= cfg->height) return fail(PTG_E_RANGE, "pixel outside the image");
    }
    if(uint64_t(jmax) / cfg->samples_per_motion_blur_step >= ctx->subframe_count)
        return fail(PTG_E_RANGE, "sample index beyond the frame's subframes");
    PTG_HIP(ctx->grow(ctx->tmp_a, n * sizeof(uint2)));
    PTG_HIP(ctx->grow(ctx->tmp_b, n * sizeof(int32_t)));
    PTG_HIP(hipMemcpyAsync(ctx->tmp_a.p, xy, n * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream));
    PTG_HIP(hipMemcpyAsync(ctx->tmp_b.p, sample_index, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    return PTG_OK;
}

int ptg_path_trace_samples(ptg_context* ctx, const ptg_render_config* cfg, size_t n, const ptg_uint2* xy,
                           const int32_t* sample_index, ptg_float4* out)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, 0)) return r;
    if(!n) return PTG_OK;
    if(!xy || !sample_index || !out || n >= (1u << 30)) return fail(PTG_E_INVALID, "ptg_path_trace_samples: bad arguments");
    if(int r = upload_sample_list(ctx, cfg, n, xy, sample_index)) return r;
    if(ctx->stack_bound >= PrivStack::kCap) return fail(PTG_E_RANGE, "walk stack bound above the per-sample kernel's stack");
    PTG_HIP(ctx->grow(ctx->tmp_c, n * sizeof(float4)));
    if(int r = launch_plain(ctx, grid_for(n), k_sample_list, ctx->scene_args(cfg), uint32_t(n), ctx->tmp_a.as<uint2>(),
                            ctx->tmp_b.as<int32_t>(), ctx->tmp_c.as<float4>()))
        return r;
    PTG_HIP(hipMemcpyAsync(out, ctx->tmp_c.p, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    return PTG_OK;
}

int ptg_trace_rays(ptg_context* ctx, uint32_t subframe, size_t n, const float* rays, uint32_t* hits)
{
    if(int r = bind(ctx)) return r;
    if(!ctx->scene_ready || !ctx->frame_ready) return fail(PTG_E_INVALID, "scene/frame not uploaded");
    if(subframe >= ctx->subframe_count) return fail(PTG_E_RANGE, "subframe out of range");
    if(!n) return PTG_OK;
    if(!rays || !hits || n >= (1u << 28)) return fail(PTG_E_INVALID, "ptg_trace_rays: bad arguments");
    // the walk's one-compare box test takes the float after tmin by +1 on its
    // bits (BlockWalker::node_block), which needs tmin's sign bit clear; the
    // reference's queries use 0 and MIN_RAY_DIST (path_tracer.hh:342, :420)
    for(size_t i = 0; i < n; ++i)
    {
        uint32_t b;
        memcpy(&b, rays + i * 8 + 6, 4);
        if((b & 0x80000000u) && (b & 0x7FFFFFFFu) <= 0x7F800000u)
            return fail(PTG_E_INVALID, "ptg_trace_rays: ray " + std::to_string(i) + " has a negative or -0 tmin (needs tmin >= +0)");
    }
    PTG_HIP(ctx->grow(ctx->tmp_a, n * 32));
    PTG_HIP(ctx->grow(ctx->tmp_b, n * 32));
    PTG_HIP(hipMemcpyAsync(ctx->tmp_a.p, rays, n * 32, hipMemcpyHostToDevice, ctx->stream));
    if(ctx->stack_bound >= PrivStack::kCap) return fail(PTG_E_RANGE, "walk stack bound above the per-ray kernels' stack");
    if(int r = launch_plain(ctx, grid_for(n), k_rays, ctx->scene_args(nullptr), ctx->host_tlas_root[subframe], uint32_t(n),
                            ctx->tmp_a.as<float>(), ctx->tmp_b.as<uint32_t>()))
        return r;
    PTG_HIP(hipMemcpyAsync(hits, ctx->tmp_b.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    return PTG_OK;
}

// The render's walk kernels over a caller's rays: one PathSoA half with the
// fields k_wf_walk reads (meta, ray_o, ray_d = nee_d), a queue of n positions
// in round `round`, an identity NEE list and a TraceOut, all in walk_state;
// then the two launches of trace_chunk_wavefront, untimed, on the context's
// stream.  Nothing of a render is touched: the streams are drained first, and
// the counters and statistics of a counted run are the call's own.
int ptg_walk_rays(ptg_context* ctx, uint32_t subframe, uint32_t round, uint32_t grid_blocks, int counted, size_t n,
                  const float* rays, uint32_t* hits, uint64_t stats[2][4])
{
    if(int r = bind(ctx)) return r;
    if(!ctx->scene_ready || !ctx->frame_ready) return fail(PTG_E_INVALID, "scene/frame not uploaded");
    if(subframe >= ctx->subframe_count) return fail(PTG_E_RANGE, "subframe out of range");
    if(round >= 255) return fail(PTG_E_RANGE, "ptg_walk_rays: round " + std::to_string(round) + " (below 255)");
    uint32_t grid[2], xcds[2];
    for(int k = 0; k < 2; ++k)
    {
        if(grid_blocks > ctx->walk_grid[k])
            return fail(PTG_E_RANGE, "ptg_walk_rays: grid_blocks " + std::to_string(grid_blocks) + " above the context's walk grid " +
                                         std::to_string(ctx->walk_grid[k]));
        grid[k] = grid_blocks ? grid_blocks : ctx->walk_grid[k];
        xcds[k] = grid_blocks ? ((grid[k] % 8 == 0 && kBands % 8 == 0) ? 8u : 1u) : ctx->walk_xcds[k];
    }
    if(counted && !stats) return fail(PTG_E_INVALID, "ptg_walk_rays: a counted run needs stats");
    if(!n) return PTG_OK;
    if(!rays || !hits || n >= (1u << 28)) return fail(PTG_E_INVALID, "ptg_walk_rays: bad arguments");
    if(ctx->host_tri_base.size() != ctx->instance_count) return fail(PTG_E_INVALID, "ptg_walk_rays: no triangle bases for this frame");
    PTG_HIP(ctx->drain());

    // walk_state: meta, origins, directions (16 B each per position), hit
    // (16), bary (8), shadow and list (4 each), then the counts and, 8-byte
    // aligned, a counted run's counters (8 per kind) and statistics
    const size_t count_words = (2 * size_t(round) + 2 + 1) & ~size_t(1);
    const size_t stat_words = 2 * (8 + kWalkWords);
    const size_t bytes = n * (3 * 16 + 16 + 8 + 4 + 4) + count_words * 4 + stat_words * 8;
    PTG_HIP(ctx->grow(ctx->walk_state, bytes));
    char* base = ctx->walk_state.as<char>();
    PathSoA S{};
    TraceOut tr{};
    S.meta = reinterpret_cast<uint4*>(base);
    S.ray_o = reinterpret_cast<float4*>(base + n * 16);
    S.ray_d = S.nee_d = reinterpret_cast<float4*>(base + n * 32);
    tr.hit = reinterpret_cast<uint4*>(base + n * 48);
    tr.bary = reinterpret_cast<float2*>(base + n * 64);
    tr.shadow = reinterpret_cast<uint32_t*>(base + n * 72);
    uint32_t* list = reinterpret_cast<uint32_t*>(base + n * 76);
    uint32_t* counts = reinterpret_cast<uint32_t*>(base + n * 80);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base + n * 80 + count_words * 4);

    std::vector<uint32_t> host, out;   // meta, origins, directions, the list, the counts; hit, bary, shadow
    try
    {
        host.assign(n * 13 + count_words, 0u);
        out.assign(n * 7, 0u);
    }
    catch(const std::bad_alloc&)
    {
        return fail(PTG_E_NOMEM, "ptg_walk_rays: host memory");
    }
    uint32_t* h_meta = host.data();
    uint32_t *h_o = h_meta + n * 4, *h_d = h_o + n * 4, *h_list = h_d + n * 4, *h_counts = h_list + n;
    // meta_pack(round, true, subframe) (a device function) and the TLAS root k_wf_camera writes
    const uint32_t meta_y = round | 0x100u | (subframe << 16), root = ctx->host_tlas_root[subframe];
    for(size_t i = 0; i < n; ++i)
    {
        const uint32_t m[4] = {uint32_t(i), meta_y, root, 0u};
        memcpy(h_meta + i * 4, m, 16);
        memcpy(h_o + i * 4, rays + i * 6, 12);
        memcpy(h_d + i * 4, rays + i * 6 + 3, 12);
        h_list[i] = uint32_t(i);
    }
    h_counts[2 * round] = h_counts[2 * round + 1] = uint32_t(n);
    hipStream_t st = ctx->stream;
    PTG_HIP(hipMemcpyAsync(base, h_meta, n * 48, hipMemcpyHostToDevice, st));
    PTG_HIP(hipMemcpyAsync(list, h_list, n * 4, hipMemcpyHostToDevice, st));
    PTG_HIP(hipMemcpyAsync(counts, h_counts, count_words * 4, hipMemcpyHostToDevice, st));
    PTG_HIP(hipMemsetAsync(cnt, 0, stat_words * 8, st));
    // a result the walks do not write keeps the sentinel: hit, bary and shadow are one range
    constexpr uint32_t kSentinel = 0xDEADBEEFu;
    PTG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(tr.hit), int(kSentinel), n * 7, st));

    const size_t region = size_t(std::max(grid[0], grid[1])) * kBlock * ctx->stack_bound;
    PTG_HIP(ctx->grow(ctx->spill, std::max<size_t>(1, 2 * region) * sizeof(uint2)));
    DevScene sc[2] = {ctx->scene_args(nullptr), ctx->scene_args(nullptr)};
    sc[0].spill = ctx->spill.as<uint2>();
    sc[1].spill = ctx->spill.as<uint2>() + region;
    unsigned long long* kc[2] = {counted ? cnt : nullptr, counted ? cnt + 8 : nullptr};
    unsigned long long* ws[2] = {counted ? cnt + 16 : nullptr, counted ? cnt + 16 + kWalkWords : nullptr};
    const uint32_t* no_list = nullptr;
    const auto closest = counted ? k_wf_walk<false, true> : k_wf_walk<false, false>;
    const auto any = counted ? k_wf_walk<true, true> : k_wf_walk<true, false>;
    hipLaunchKernelGGL(closest, dim3(grid[0]), dim3(kBlock), ctx->walk_lds[0], st, sc[0], S, counts, round, no_list, tr, xcds[0],
                       kc[0], ws[0]);
    PTG_HIP(hipGetLastError());
    hipLaunchKernelGGL(any, dim3(grid[1]), dim3(kBlock), ctx->walk_lds[1], st, sc[1], S, counts, round, list, tr, xcds[1], kc[1],
                       ws[1]);
    PTG_HIP(hipGetLastError());

    unsigned long long h_stats[2 * (8 + kWalkWords)];
    PTG_HIP(hipMemcpyAsync(out.data(), tr.hit, n * 28, hipMemcpyDeviceToHost, st));
    PTG_HIP(hipMemcpyAsync(h_stats, cnt, sizeof(h_stats), hipMemcpyDeviceToHost, st));
    PTG_HIP(hipStreamSynchronize(st));
    const uint32_t *o_hit = out.data(), *o_bary = o_hit + n * 4, *o_shadow = o_bary + n * 2;
    for(size_t i = 0; i < n; ++i)
    {
        const uint32_t* h = o_hit + i * 4;
        const bool miss = h[1] == 0xFFFFFFFFu;
        if(h[0] == kSentinel || o_shadow[i] == kSentinel || (!miss && o_bary[2 * i] == kSentinel && o_bary[2 * i + 1] == kSentinel))
            return fail(PTG_E_RANGE, "ptg_walk_rays: queue position " + std::to_string(i) + " of " + std::to_string(n) +
                                         " was not written by the " + (o_shadow[i] == kSentinel ? "any-hit" : "closest-hit") +
                                         " walk (grid " + std::to_string(grid[0]) + " / " + std::to_string(grid[1]) + ")");
        if(!miss && (h[1] >= ctx->instance_count || h[2] < ctx->host_tri_base[h[1]]))
            return fail(PTG_E_RANGE, "ptg_walk_rays: position " + std::to_string(i) + " names instance " + std::to_string(h[1]) +
                                         ", triangle " + std::to_string(h[2]));
        uint32_t* w = hits + i * 8;
        w[0] = miss ? 0u : o_bary[2 * i];
        w[1] = miss ? 0u : o_bary[2 * i + 1];
        w[2] = 0u;
        w[3] = h[0];
        w[4] = h[1];
        w[5] = miss ? h[2] : h[2] - ctx->host_tri_base[h[1]];   // mesh-global -> mesh-local
        w[6] = h[3];
        w[7] = o_shadow[i];
    }
    if(stats)
        for(int k = 0; k < 2; ++k)
            for(int j = 0; j < WX_COUNT; ++j) stats[k][j] = counted ? h_stats[16 + k * kWalkWords + WS_COUNT + j] : 0;
    // a lane's spill area holds stack_bound 8-byte entries: 2 * stack_bound slots of a slot stack
    const uint64_t room[2] = {uint64_t(ctx->stack_bound) * (std::is_same<WalkStackOf<false>::type, LdsStack>::value ? 1 : 2),
                              uint64_t(ctx->stack_bound) * (std::is_same<WalkStackOf<true>::type, LdsStack>::value ? 1 : 2)};
    for(int k = 0; counted && k < 2; ++k)
        if(stats[k][WX_MAX_SIZE] > room[k])
            return fail(PTG_E_RANGE, std::string("ptg_walk_rays: the ") + (k ? "any-hit" : "closest-hit") + " walk's stack reached " +
                                         std::to_string(stats[k][WX_MAX_SIZE]) + ", its spill area holds " + std::to_string(room[k]));
    return PTG_OK;
}

int ptg_camera_rays(ptg_context* ctx, const ptg_render_config* cfg, size_t n, const ptg_uint2* xy,
                    const int32_t* sample_index, float* rays, uint32_t* subframe)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, 0)) return r;
    if(!n) return PTG_OK;
    if(!xy || !sample_index || !rays || !subframe || n >= (1u << 28)) return fail(PTG_E_INVALID, "ptg_camera_rays: bad arguments");
    if(int r = upload_sample_list(ctx, cfg, n, xy, sample_index)) return r;
    PTG_HIP(ctx->grow(ctx->tmp_c, n * 36));            // n rays of 8 floats, then n subframe indices
    float* d_rays = ctx->tmp_c.as<float>();
    uint32_t* d_sub = reinterpret_cast<uint32_t*>(d_rays + n * 8);
    if(int r = launch_plain(ctx, grid_for(n), k_camera_rays, ctx->scene_args(cfg), uint32_t(n), ctx->tmp_a.as<uint2>(),
                            ctx->tmp_b.as<int32_t>(), d_rays, d_sub))
        return r;
    PTG_HIP(hipMemcpyAsync(rays, d_rays, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    PTG_HIP(hipMemcpyAsync(subframe, d_sub, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    return PTG_OK;
}

// The feature pass over the pixels of `pm` (a rectangle or a tile set), its arguments checked.
static int features_map(ptg_context* ctx, const ptg_render_config* cfg, const PixelMap& pm, uint32_t sample_begin,
                        uint32_t sample_end, ptg_float4* out_albedo, ptg_float4* out_normal_depth)
{
    // persistent blocks, each taking groups of kBlock / 8 pixels (4 waves of 8
    // pixels x 8 samples); every walk lane owns stack_bound entries of spill
    const uint32_t grid = std::min<uint32_t>(grid_for(pm.npix, kBlock / 8), std::max(1u, ctx->persistent_blocks / 4u));   // 8 per CU
    PTG_HIP(ctx->grow(ctx->feat_spill, std::max<size_t>(1, size_t(grid) * kBlock * ctx->stack_bound) * sizeof(uint2)));
    DevScene sc = ctx->scene_args(cfg);
    sc.spill = ctx->feat_spill.as<uint2>();
    return launch_plain(ctx, grid, k_features, sc, pm, sample_begin, sample_end, (float)cfg->samples_per_pixel,
                        reinterpret_cast<float4*>(out_albedo), reinterpret_cast<float4*>(out_normal_depth));
}

// All five planes of `out` (the feature planes given) over the pixels of `pm`:
// one fused render on the wavefront pipeline; the megakernel keeps no path
// state between kernels, so there the render without the feature planes, then
// the feature pass - the same bits.
static int render_planes(ptg_context* ctx, const ptg_render_config* cfg, const PixelMap& pm, uint32_t j0, uint32_t j1,
                         const Planes& out)
{
    if(ctx->pipeline == 0) return render_map(ctx, cfg, pm, j0, j1, out);
    if(int r = render_map(ctx, cfg, pm, j0, j1, Planes{out.accum, out.bgra, out.moments})) return r;
    return features_map(ctx, cfg, pm, j0, j1, out.albedo, out.normal_depth);
}

// check_planes' verdict (host/planes.h) as an entry's return: the message set where it refuses
static int refused(const PlanesVerdict& v) { return v.code == PTG_OK ? PTG_OK : fail(v.code, v.message); }

int ptg_render_features(ptg_context* ctx, const ptg_render_config* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                        uint32_t sample_begin, uint32_t sample_end, ptg_float4* out_albedo, ptg_float4* out_normal_depth)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, sample_end)) return r;
    PixelMap pm;
    if(int r = rect_map(cfg, x0, y0, w, h, pm)) return r;
    if(pm.npix == 0) return PTG_OK;
    if(!out_albedo || !out_normal_depth) return fail(PTG_E_INVALID, "ptg_render_features: null output");
    if(sample_end <= sample_begin) return fail(PTG_E_INVALID, "empty sample range");
    return features_map(ctx, cfg, pm, sample_begin, sample_end, out_albedo, out_normal_depth);
}

int ptg_render_with_features(ptg_context* ctx, const ptg_render_config* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                             uint32_t sample_begin, uint32_t sample_end, ptg_float4* out_accum, ptg_uchar4* out_bgra,
                             ptg_float4* out_moments, ptg_float4* out_albedo, ptg_float4* out_normal_depth)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, sample_end)) return r;
    if(!out_albedo || !out_normal_depth) return fail(PTG_E_INVALID, "ptg_render_with_features: null feature output");
    const Planes out{out_accum, out_bgra, out_moments, out_albedo, out_normal_depth};
    if(int r = refused(check_planes("ptg_render_with_features", out, 0, nullptr, false, false))) return r;
    PixelMap pm;
    if(int r = rect_map(cfg, x0, y0, w, h, pm)) return r;
    if(pm.npix == 0) return PTG_OK;
    if(sample_end <= sample_begin) return fail(PTG_E_INVALID, "empty sample range");
    return render_planes(ctx, cfg, pm, sample_begin, sample_end, out);
}

// ---- tile packs: a tile shard's five planes in one buffer (ptg.h; carved by host/planes.h) ----

size_t ptg_tile_pack_bytes(uint32_t tile_w, uint32_t tile_h, uint32_t pack_tiles)
{
    return tile_pack_bytes(tile_pack_slots(tile_w, tile_h, pack_tiles));
}

int ptg_render_tiles_packed(ptg_context* ctx, const ptg_render_config* cfg, uint32_t tile_w, uint32_t tile_h,
                            uint32_t first_tile, uint32_t tile_stride, uint32_t tile_count, uint32_t pack_tiles, void* pack)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, cfg ? cfg->samples_per_pixel : 0)) return r;
    if(pack_tiles < tile_count)
        return fail(PTG_E_INVALID, "ptg_render_tiles_packed: a pack of " + std::to_string(pack_tiles) + " tiles for " +
                                       std::to_string(tile_count));
    if(!pack) return fail(PTG_E_INVALID, "ptg_render_tiles_packed: null pack");
    if(reinterpret_cast<uintptr_t>(pack) % sizeof(float4)) return fail(PTG_E_INVALID, "ptg_render_tiles_packed: the pack is not 16-byte aligned");
    PixelMap pm;
    if(int r = tile_map(cfg, tile_w, tile_h, first_tile, tile_stride, tile_count, pm)) return r;
    if(pack_tiles == 0) return PTG_OK;   // no tile and no byte
    const uint64_t slots = tile_pack_slots(tile_w, tile_h, pack_tiles);
    if(slots == 0) return fail(PTG_E_RANGE, "ptg_render_tiles_packed: too many pack slots");
    // everything the render does not write - pixels outside the image in the
    // feature planes, the tiles behind tile_count, the padding - is 0
    PTG_HIP(hipMemsetAsync(pack, 0, tile_pack_bytes(slots), ctx->stream));
    if(pm.npix == 0) return PTG_OK;
    return render_planes(ctx, cfg, pm, 0, cfg->samples_per_pixel, pack_planes(pack, slots));
}

int ptg_assemble_tile_packs(ptg_context* ctx, const ptg_render_config* cfg, uint32_t tile_w, uint32_t tile_h, uint32_t world,
                            uint32_t pack_tiles, const void* packs, ptg_float4* out_accum, ptg_uchar4* out_bgra,
                            ptg_float4* out_moments, ptg_float4* out_albedo, ptg_float4* out_normal_depth)
{
    if(int r = bind(ctx)) return r;
    if(!cfg || cfg->width == 0 || cfg->height == 0) return fail(PTG_E_INVALID, "bad render config");
    const uint64_t npix = uint64_t(cfg->width) * cfg->height;
    if(npix >= (1ull << 31)) return fail(PTG_E_RANGE, "image too large");
    if(tile_w == 0 || tile_h == 0) return fail(PTG_E_INVALID, "bad tile geometry");
    if(world == 0) return fail(PTG_E_INVALID, "ptg_assemble_tile_packs: world size 0");
    if(!packs) return fail(PTG_E_INVALID, "ptg_assemble_tile_packs: null packs");
    if(reinterpret_cast<uintptr_t>(packs) % sizeof(float4)) return fail(PTG_E_INVALID, "ptg_assemble_tile_packs: the packs are not 16-byte aligned");
    const uint32_t tiles_x = (cfg->width + tile_w - 1) / tile_w, tiles_y = (cfg->height + tile_h - 1) / tile_h;
    const uint64_t need = (uint64_t(tiles_x) * tiles_y + world - 1) / world;
    if(pack_tiles < need)
        return fail(PTG_E_RANGE, "ptg_assemble_tile_packs: packs of " + std::to_string(pack_tiles) + " tiles, the largest rank holds " +
                                     std::to_string(need));
    const uint64_t slots = tile_pack_slots(tile_w, tile_h, pack_tiles);
    if(slots == 0) return fail(PTG_E_RANGE, "ptg_assemble_tile_packs: too many pack slots");
    const size_t pack_bytes = tile_pack_bytes(slots);
    const Planes out{out_accum, out_bgra, out_moments, out_albedo, out_normal_depth};
    const ForbiddenRange gathered{packs, size_t(world) * pack_bytes, "overlaps the packs"};
    if(int r = refused(check_planes("ptg_assemble_tile_packs", out, npix, &gathered, true, true))) return r;
    return launch_plain(ctx, grid_for(npix), k_assemble_tile_packs, cfg->width, uint32_t(npix), tile_w, tile_h, tiles_x, world,
                        uint32_t(slots), pack_bytes, static_cast<const uint8_t*>(packs), out);
}

// ---- progressive rendering (ptg_accum_*) ----

static uint32_t accum_plane_count(uint32_t flags)
{
    return 1u + (flags & PTG_ACCUM_MOMENTS ? 1u : 0u) + (flags & PTG_ACCUM_FEATURES ? 2u : 0u);
}

size_t ptg_accum_state_bytes(uint32_t w, uint32_t h, uint32_t flags)
{
    if(flags & ~(PTG_ACCUM_MOMENTS | PTG_ACCUM_FEATURES)) return 0;
    return size_t(accum_plane_count(flags)) * w * h * sizeof(float4);
}

// A header ptg_accum_begin could have written (it may come from a file).
static int check_accum(const char* who, const ptg_accum* acc, const void* state)
{
    const std::string w(who);
    if(!acc || !state) return fail(PTG_E_INVALID, w + ": null header or state");
    if(acc->magic != PTG_ACCUM_MAGIC || acc->version != PTG_ACCUM_VERSION)
        return fail(PTG_E_INVALID, w + ": not a ptg_accum header (bad magic or version)");
    if(acc->flags & ~(PTG_ACCUM_MOMENTS | PTG_ACCUM_FEATURES)) return fail(PTG_E_INVALID, w + ": unknown flag bits");
    if(acc->sample_next < acc->sample_begin) return fail(PTG_E_INVALID, w + ": the header's sample range runs backwards");
    return PTG_OK;
}

// The sums of a state with the header's rectangle and flags.
static Sums accum_sums(const ptg_accum& acc, void* state)
{
    const size_t npix = size_t(acc.w) * acc.h;
    Sums pl;
    ptg_float4* next = static_cast<ptg_float4*>(state);
    pl.acc = next;
    next += npix;
    if(acc.flags & PTG_ACCUM_MOMENTS)
    {
        pl.mom = next;
        next += npix;
    }
    if(acc.flags & PTG_ACCUM_FEATURES) pl.feat = next;
    return pl;
}

int ptg_accum_begin(ptg_context* ctx, const ptg_render_config* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                    uint32_t flags, uint32_t sample_begin, ptg_accum* acc, void* state)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_cfg(ctx, cfg, sample_begin)) return r;
    if(!acc || !state) return fail(PTG_E_INVALID, "ptg_accum_begin: null header or state");
    if(flags & ~(PTG_ACCUM_MOMENTS | PTG_ACCUM_FEATURES)) return fail(PTG_E_INVALID, "ptg_accum_begin: unknown flag bits");
    PixelMap pm;
    if(int r = rect_map(cfg, x0, y0, w, h, pm)) return r;
    if(pm.npix) PTG_HIP(hipMemsetAsync(state, 0, ptg_accum_state_bytes(w, h, flags), ctx->stream));
    *acc = ptg_accum{PTG_ACCUM_MAGIC, PTG_ACCUM_VERSION, *cfg, x0, y0, w, h, flags, sample_begin, sample_begin, 0u};
    return PTG_OK;
}

int ptg_accum_add(ptg_context* ctx, ptg_accum* acc, void* state, uint32_t sample_end)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_accum("ptg_accum_add", acc, state)) return r;
    if(sample_end <= acc->sample_next)
        return fail(PTG_E_INVALID, "ptg_accum_add: sample_end " + std::to_string(sample_end) + " adds nothing to a state that holds samples up to " +
                                       std::to_string(acc->sample_next));
    const ptg_render_config cfg = acc->cfg;
    if(int r = check_cfg(ctx, &cfg, sample_end)) return r;
    PixelMap pm;
    if(int r = rect_map(&cfg, acc->x0, acc->y0, acc->w, acc->h, pm)) return r;
    if((acc->flags & PTG_ACCUM_FEATURES) && ctx->pipeline != 0)
        return fail(PTG_E_INVALID, "ptg_accum_add: PTG_ACCUM_FEATURES runs on the wavefront pipeline only (ptg_set_pipeline(ctx, 0))");
    const Sums sums = accum_sums(*acc, state);
    if(int r = render_map(ctx, &cfg, pm, acc->sample_next, sample_end, Planes{}, &sums)) return r;
    acc->sample_next = sample_end;
    return PTG_OK;
}

int ptg_accum_resolve(ptg_context* ctx, const ptg_accum* acc, const void* state, int by_samples, ptg_float4* out_accum,
                      ptg_uchar4* out_bgra, ptg_float4* out_moments, ptg_float4* out_albedo, ptg_float4* out_normal_depth)
{
    if(int r = bind(ctx)) return r;
    if(int r = check_accum("ptg_accum_resolve", acc, state)) return r;
    if(acc->sample_next == acc->sample_begin) return fail(PTG_E_INVALID, "ptg_accum_resolve: the state holds no sample");
    if(acc->cfg.samples_per_pixel == 0) return fail(PTG_E_INVALID, "bad render config");
    if(out_moments && !(acc->flags & PTG_ACCUM_MOMENTS))
        return fail(PTG_E_INVALID, "ptg_accum_resolve: out_moments of a state without PTG_ACCUM_MOMENTS");
    if((out_albedo || out_normal_depth) && !(acc->flags & PTG_ACCUM_FEATURES))
        return fail(PTG_E_INVALID, "ptg_accum_resolve: a feature output of a state without PTG_ACCUM_FEATURES");
    const size_t npix = size_t(acc->w) * acc->h;
    if(npix >= (1ull << 31)) return fail(PTG_E_RANGE, "image too large");
    const Planes out{out_accum, out_bgra, out_moments, out_albedo, out_normal_depth};
    const ForbiddenRange planes{state, ptg_accum_state_bytes(acc->w, acc->h, acc->flags), "lies inside the state"};
    if(int r = refused(check_planes("ptg_accum_resolve", out, npix, &planes, true, false))) return r;
    if(npix == 0) return PTG_OK;
    const float div = by_samples ? (float)(acc->sample_next - acc->sample_begin) : (float)acc->cfg.samples_per_pixel;
    return launch_plain(ctx, grid_for(npix), k_resolve<false>, uint32_t(npix), accum_sums(*acc, const_cast<void*>(state)), div,
                        out, static_cast<uint32_t*>(nullptr));
}

int ptg_last_counters(ptg_context* ctx, uint64_t out[8])
{
    if(!ctx || !out) return fail(PTG_E_INVALID, "ptg_last_counters: bad arguments");
    if(!ctx->counting) return fail(PTG_E_INVALID, "counters disabled (ptg_counters_enable)");
    memcpy(out, ctx->last_counters, sizeof(ctx->last_counters));
    return PTG_OK;
}

int ptg_counters_enable(ptg_context* ctx, int enable)
{
    if(!ctx) return fail(PTG_E_INVALID, "null context");
    ctx->counting = enable != 0;
    return PTG_OK;
}

int ptg_timing_enable(ptg_context* ctx, int enable)
{
    if(!ctx) return fail(PTG_E_INVALID, "null context");
    ctx->timing = enable != 0;
    ctx->ev_used = 0;
    return PTG_OK;
}

// a recorded launch's device interval: start and end on one time axis
// (relative to the first recorded start), and its length as the events give it
struct Interval { int kind; double s, e, ms; };

// The intervals of the launches recorded since timing was enabled or last
// read, in recording order; waits for them and clears the record.
static int take_intervals(ptg_context* ctx, std::vector<Interval>& iv)
{
    iv.clear();
    iv.reserve(ctx->ev_used);
    for(size_t i = 0; i < ctx->ev_used; ++i)
    {
        PTG_HIP(hipEventSynchronize(ctx->ev_stop[i]));
        float s = 0, e = 0, t = 0;
        PTG_HIP(hipEventElapsedTime(&s, ctx->ev_start[0], ctx->ev_start[i]));
        PTG_HIP(hipEventElapsedTime(&e, ctx->ev_start[0], ctx->ev_stop[i]));
        PTG_HIP(hipEventElapsedTime(&t, ctx->ev_start[i], ctx->ev_stop[i]));
        iv.push_back(Interval{ctx->ev_kind[i], double(s), double(e), double(t)});
    }
    ctx->ev_used = 0;
    return PTG_OK;
}

int ptg_last_kernel_times(ptg_context* ctx, double ms[8], uint32_t launches[8])
{
    if(int r = bind(ctx)) return r;
    if(!ms || !launches) return fail(PTG_E_INVALID, "ptg_last_kernel_times: bad arguments");
    std::vector<Interval> iv;
    if(int r = take_intervals(ctx, iv)) return r;
    for(int k = 0; k < 8; ++k) { ms[k] = 0; launches[k] = 0; }
    for(const Interval& v: iv)
    {
        ms[v.kind] += v.ms;
        launches[v.kind] += 1;
    }
    return PTG_OK;
}

int ptg_last_kernel_busy(ptg_context* ctx, double busy_ms[8], double ms[8], uint32_t launches[8])
{
    if(int r = bind(ctx)) return r;
    if(!busy_ms || !ms || !launches) return fail(PTG_E_INVALID, "ptg_last_kernel_busy: bad arguments");
    std::vector<Interval> iv;
    if(int r = take_intervals(ctx, iv)) return r;
    std::sort(iv.begin(), iv.end(), [](const Interval& a, const Interval& b) { return a.s < b.s; });
    for(int k = 0; k < 8; ++k)
    {
        busy_ms[k] = ms[k] = 0;
        launches[k] = 0;
        bool open = false;        // a merged interval [cs, ce] of kind k is open
        double cs = 0, ce = 0;
        for(const Interval& v: iv)
        {
            if(v.kind != k) continue;
            ms[k] += v.e - v.s;
            launches[k] += 1;
            if(!open || v.s > ce)
            {
                if(open) busy_ms[k] += ce - cs;
                cs = v.s;
                ce = v.e;
                open = true;
            }
            else ce = std::max(ce, v.e);
        }
        if(open) busy_ms[k] += ce - cs;
    }
    return PTG_OK;
}

int ptg_last_timing(ptg_context* ctx, double* trace_ms, uint32_t* launches)
{
    if(!trace_ms || !launches) return fail(PTG_E_INVALID, "ptg_last_timing: bad arguments");
    double ms[8];
    uint32_t n[8];
    if(int r = ptg_last_kernel_times(ctx, ms, n)) return r;
    *trace_ms = 0;
    *launches = 0;
    for(int k = 0; k < 8; ++k)
        if(k != K_ACCUM) { *trace_ms += ms[k]; *launches += n[k]; }
    return PTG_OK;
}

int ptg_last_kernel_counters(ptg_context* ctx, uint64_t out[6][8])
{
    if(!ctx || !out) return fail(PTG_E_INVALID, "ptg_last_kernel_counters: bad arguments");
    if(!ctx->counting) return fail(PTG_E_INVALID, "counters disabled (ptg_counters_enable)");
    memcpy(out, ctx->kind_counters, sizeof(ctx->kind_counters));
    return PTG_OK;
}

int ptg_last_redo_stats(ptg_context* ctx, uint64_t out[9])
{
    if(!ctx || !out) return fail(PTG_E_INVALID, "ptg_last_redo_stats: bad arguments");
    if(!ctx->counting) return fail(PTG_E_INVALID, "counters disabled (ptg_counters_enable)");
    static_assert(kRedoWords == 9, "ptg.h documents 9 words");
    memcpy(out, ctx->redo_stats, sizeof(ctx->redo_stats));
    return PTG_OK;
}

int ptg_last_walk_stats(ptg_context* ctx, uint64_t out[2][8])
{
    if(!ctx || !out) return fail(PTG_E_INVALID, "ptg_last_walk_stats: bad arguments");
    if(!ctx->counting) return fail(PTG_E_INVALID, "counters disabled (ptg_counters_enable)");
    static_assert(WS_COUNT == 8, "ptg.h documents 8 walk statistics");
    memcpy(out, ctx->walk_stats, sizeof(ctx->walk_stats));
    return PTG_OK;
}

int ptg_set_hbm_share(ptg_context* ctx, int percent)
{
    if(!ctx || percent < 5 || percent > 70) return fail(PTG_E_INVALID, "ptg_set_hbm_share: 5 .. 70 percent");
    ctx->hbm_pct = uint32_t(percent);
    return PTG_OK;
}

int ptg_set_chunk_paths(ptg_context* ctx, int log2_paths)
{
    if(!ctx || log2_paths < 16 || log2_paths > 28) return fail(PTG_E_INVALID, "ptg_set_chunk_paths: 16 .. 28");
    ctx->chunk_log2 = uint32_t(log2_paths);
    return PTG_OK;
}

int ptg_set_concurrency(ptg_context* ctx, int level)
{
    if(!ctx || level < 0 || level > 2) return fail(PTG_E_INVALID, "ptg_set_concurrency: 0, 1 or 2");
    ctx->concurrency = uint32_t(level);
    return PTG_OK;
}

int ptg_set_pipeline(ptg_context* ctx, int pipeline)
{
    if(!ctx || pipeline < 0 || pipeline > 1) return fail(PTG_E_INVALID, "ptg_set_pipeline: 0 = wavefront, 1 = megakernel");
    ctx->pipeline = pipeline;
    return PTG_OK;
}

int ptg_arith_selftest(ptg_context* ctx)
{
    if(int r = bind(ctx)) return r;
    const int m = ptg_device_selftest(ctx->stream);
    if(m < 0) return fail(PTG_E_HIP, std::string("ptg_arith_selftest: ") + hipGetErrorString(hipError_t(-m)));
    return m;
}

int ptg_synchronize(ptg_context* ctx)
{
    if(int r = bind(ctx)) return r;
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    return PTG_OK;
}

int ptg_device_alloc(ptg_context* ctx, size_t bytes, void** out)
{
    if(int r = bind(ctx)) return r;
    if(!out) return fail(PTG_E_INVALID, "null out");
    PTG_HIP(hipMalloc(out, bytes));
    return PTG_OK;
}

int ptg_device_free(ptg_context* ctx, void* p)
{
    if(int r = bind(ctx)) return r;
    PTG_HIP(hipFree(p));
    return PTG_OK;
}

int ptg_memcpy_d2h(ptg_context* ctx, void* dst, const void* src, size_t bytes)
{
    if(int r = bind(ctx)) return r;
    PTG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    return PTG_OK;
}

} // extern "C"
