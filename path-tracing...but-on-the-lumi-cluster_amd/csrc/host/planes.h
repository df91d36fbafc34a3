// A frame's plane set, from the C entries to the kernels: the five outputs,
// the three running sums they are closed from, the one check of caller-given
// outputs, and the carving of a tile pack (include/ptg.h) into its planes.
//
//   Planes, Sums            PODs, passed to kernels by value
//   check_planes()          distinct, present, aligned, outside a byte range
//   tile_pack_slots(), tile_pack_bytes(), pack_planes()
//
// Only ptg.h's types and no HIP call: every HIP unit includes it, and so does
// a host-only program (tests/plane_set).
#pragma once
#include "ptg.h"
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define PTG_PLANES_HD __host__ __device__
#else
#define PTG_PLANES_HD
#endif

namespace ptg {

// The five outputs of a frame, in the entries' argument order; each may be null.
struct Planes {
    ptg_float4* accum = nullptr;          // radiance
    ptg_uchar4* bgra = nullptr;           // its tonemap
    ptg_float4* moments = nullptr;        // (m1, m2, variance of the mean, n)
    ptg_float4* albedo = nullptr;         // albedo + coverage
    ptg_float4* normal_depth = nullptr;   // normal + depth
};
constexpr int kPlanes = 5;

// The running per-pixel sums the planes are closed from: the context's own
// (acc, mom, feat_acc) in a one-shot render, the caller's state planes in a
// progressive one (ptg.h's state layout).  mom and feat are null where the
// render, or the state, carries no such sums.
struct Sums {
    ptg_float4* acc = nullptr;    // the radiance sums
    ptg_float4* mom = nullptr;    // (s1, s2, n as bits, 0)
    ptg_float4* feat = nullptr;   // two planes: albedo + coverage, normal + depth
};

// A byte range no output may touch, and the words to say about one that does
// ("<entry>: an output <words>").
struct ForbiddenRange {
    const void* base;
    size_t bytes;
    const char* words;
};

struct PlanesVerdict {
    int code = PTG_OK;
    std::string message;
};

// The check of an entry's caller-given outputs of `npix` pixels each.  Per
// output, in the order of Planes: its alignment (`aligned`: 16 bytes, bgra 4),
// that no later output is the same buffer, that it stays outside `forbidden`
// (null: no such range); then, with `need_one`, that there is an output at
// all.  The first rule broken gives the verdict.  Addresses are compared as
// integers: the pointers are the caller's device pointers and are not followed.
// (static: the library exports no symbol for it.)
static inline PlanesVerdict check_planes(const char* entry, const Planes& out, uint64_t npix, const ForbiddenRange* forbidden,
                                  bool need_one, bool aligned)
{
    const uintptr_t at[kPlanes] = {reinterpret_cast<uintptr_t>(out.accum), reinterpret_cast<uintptr_t>(out.bgra),
                                   reinterpret_cast<uintptr_t>(out.moments), reinterpret_cast<uintptr_t>(out.albedo),
                                   reinterpret_cast<uintptr_t>(out.normal_depth)};
    const auto refuse = [&](const std::string& what) { return PlanesVerdict{PTG_E_INVALID, std::string(entry) + ": " + what}; };
    bool any = false;
    for(int a = 0; a < kPlanes; ++a)
    {
        if(!at[a]) continue;
        any = true;
        const uint64_t elem = a == 1 ? sizeof(ptg_uchar4) : sizeof(ptg_float4);
        if(aligned && at[a] % elem) return refuse("a misaligned output");
        for(int b = a + 1; b < kPlanes; ++b)
            if(at[a] == at[b]) return refuse("two outputs are the same buffer");
        if(!forbidden) continue;
        // [at, at + npix * elem) against [lo, lo + bytes), without forming either end
        const uintptr_t lo = reinterpret_cast<uintptr_t>(forbidden->base);
        const bool touches = at[a] >= lo ? at[a] - lo < forbidden->bytes : lo - at[a] < npix * elem;
        if(touches) return refuse(std::string("an output ") + forbidden->words);
    }
    if(need_one && !any) return refuse("no output given");
    return PlanesVerdict{};
}

// ---- tile packs (ptg.h): four float4 planes, then the uchar4 plane ----

// The slots of a pack, 0 when a dimension is 0 or they do not stay below 2^31.
inline uint64_t tile_pack_slots(uint32_t tw, uint32_t th, uint32_t pack_tiles)
{
    const uint64_t per = uint64_t(tw) * th;
    if(per == 0 || pack_tiles == 0 || per >= (1ull << 31)) return 0;
    const uint64_t slots = per * pack_tiles;   // below 2^63
    return slots < (1ull << 31) ? slots : 0;
}

// A pack's bytes, which is also the stride between gathered packs: padded to 256.
inline size_t tile_pack_bytes(uint64_t slots)
{
    return size_t((slots * (4 * sizeof(ptg_float4) + sizeof(ptg_uchar4)) + 255u) & ~uint64_t(255));
}

// The planes of the pack of `slots` slots at `base`, for the render that
// writes it and the assembly that reads it.
PTG_PLANES_HD inline Planes pack_planes(void* base, size_t slots)
{
    ptg_float4* const f = static_cast<ptg_float4*>(base);
    Planes pl;
    pl.accum = f;
    pl.moments = f + slots;
    pl.albedo = f + 2 * slots;
    pl.normal_depth = f + 3 * slots;
    pl.bgra = reinterpret_cast<ptg_uchar4*>(f + 4 * slots);
    return pl;
}

} // namespace ptg
