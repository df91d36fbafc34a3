// CPU test of the plane set's host half (csrc/host/planes.h): check_planes, the
// one check of an entry's caller-given outputs, and the carving of a tile pack
// against include/ptg.h's stated layout.  No GPU, no HIP: the outputs are
// addresses that nothing follows.
//
//   plane_set_test        every rule alone, every pair of rules at once, the
//                         forbidden range at its ends, bgra's element size,
//                         the pack's planes and bytes, the refusals at 2^31
//
// Built with -DPLANE_SET_NO_LIB (make plane_set_test_host) it needs no
// libptg.so - the build for a sanitizer run - and leaves out only the
// comparison with the exported ptg_tile_pack_bytes.
#include "ptg.h"
#include "host/planes.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

using namespace ptg;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if(!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while(0)

static_assert(std::is_trivially_copyable<Planes>::value && std::is_trivially_copyable<Sums>::value, "passed to kernels by value");
static_assert(sizeof(Planes) == 5 * sizeof(void*) && sizeof(Sums) == 3 * sizeof(void*), "five outputs, three sums");

// addresses as outputs: never dereferenced
ptg_float4* f4(uintptr_t a) { return reinterpret_cast<ptg_float4*>(a); }
ptg_uchar4* u4(uintptr_t a) { return reinterpret_cast<ptg_uchar4*>(a); }

constexpr uintptr_t kBase = 0x40000000u;   // the forbidden range's first byte
constexpr size_t kRange = 4096;            // its bytes
constexpr uint64_t kPix = 10;              // pixels per output: 160 bytes, bgra 40
constexpr uintptr_t kFar = 0x10000000u;    // well away from the range; kFar + 0x1000 * k: distinct aligned buffers
const ForbiddenRange kForbidden{reinterpret_cast<const void*>(kBase), kRange, "overlaps the packs"};

Planes all_far()
{
    return Planes{f4(kFar), u4(kFar + 0x1000), f4(kFar + 0x2000), f4(kFar + 0x3000), f4(kFar + 0x4000)};
}

// the verdict of the full check (range, one output needed, alignment) as "code message"
std::string full(const Planes& p, const char* entry = "E")
{
    const PlanesVerdict v = check_planes(entry, p, kPix, &kForbidden, true, true);
    return std::to_string(v.code) + " " + v.message;
}

const std::string kOk = "0 ";
const std::string kMisaligned = "-1 E: a misaligned output";
const std::string kSame = "-1 E: two outputs are the same buffer";
const std::string kRangeMsg = "-1 E: an output overlaps the packs";
const std::string kNone = "-1 E: no output given";

void test_rules_alone()
{
    CHECK(PTG_E_INVALID == -1 && PTG_OK == 0);
    CHECK(full(all_far()) == kOk);
    // one output only, each of the five
    for(int k = 0; k < 5; ++k)
    {
        Planes p;
        if(k == 0) p.accum = f4(kFar);
        if(k == 1) p.bgra = u4(kFar);
        if(k == 2) p.moments = f4(kFar);
        if(k == 3) p.albedo = f4(kFar);
        if(k == 4) p.normal_depth = f4(kFar);
        CHECK(full(p) == kOk);
    }
    // all five null: refused only where one is needed
    CHECK(full(Planes{}) == kNone);
    CHECK(check_planes("E", Planes{}, kPix, &kForbidden, false, true).code == PTG_OK);
    CHECK(check_planes("E", Planes{}, kPix, nullptr, false, false).code == PTG_OK);
    // misaligned, each output alone
    for(int k = 0; k < 5; ++k)
    {
        Planes p = all_far();
        if(k == 0) p.accum = f4(kFar + 8);
        if(k == 1) p.bgra = u4(kFar + 0x1000 + 2);
        if(k == 2) p.moments = f4(kFar + 0x2000 + 4);
        if(k == 3) p.albedo = f4(kFar + 0x3000 + 1);
        if(k == 4) p.normal_depth = f4(kFar + 0x4000 + 12);
        CHECK(full(p) == kMisaligned);
        // not asked: not a rule
        CHECK(check_planes("E", p, kPix, &kForbidden, true, false).code == PTG_OK);
    }
    // the same buffer, every pair of outputs (bgra's address under a float4 name and the other way)
    for(int a = 0; a < 5; ++a)
        for(int b = a + 1; b < 5; ++b)
        {
            uintptr_t at[5] = {kFar, kFar + 0x1000, kFar + 0x2000, kFar + 0x3000, kFar + 0x4000};
            at[b] = at[a];
            const Planes p{f4(at[0]), u4(at[1]), f4(at[2]), f4(at[3]), f4(at[4])};
            CHECK(full(p) == kSame);
            CHECK(check_planes("E", p, kPix, nullptr, false, false).message == "E: two outputs are the same buffer");
        }
    // two null outputs are not "the same buffer"
    CHECK(full(Planes{f4(kFar), nullptr, nullptr, f4(kFar + 0x1000), nullptr}) == kOk);
    // inside the range, each output alone; without a range: not a rule
    for(int k = 0; k < 5; ++k)
    {
        Planes p = all_far();
        if(k == 0) p.accum = f4(kBase + 16);
        if(k == 1) p.bgra = u4(kBase + 16);
        if(k == 2) p.moments = f4(kBase + 16);
        if(k == 3) p.albedo = f4(kBase + 16);
        if(k == 4) p.normal_depth = f4(kBase + 16);
        CHECK(full(p) == kRangeMsg);
        CHECK(check_planes("E", p, kPix, nullptr, true, true).code == PTG_OK);
    }
    // the entry's name and the range's words are the caller's
    const ForbiddenRange state{reinterpret_cast<const void*>(kBase), kRange, "lies inside the state"};
    const PlanesVerdict v = check_planes("ptg_accum_resolve", Planes{f4(kBase)}, kPix, &state, true, false);
    CHECK(v.code == PTG_E_INVALID && v.message == "ptg_accum_resolve: an output lies inside the state");
}

// Two rules broken at once: per output, in the order of Planes, alignment,
// then the same buffer, then the range; so the earlier output's rule wins, and
// on one output the earlier rule.  ("No output given" cannot be broken
// together with another rule: with no output there is nothing to misalign,
// repeat or place.)
void test_rule_pairs()
{
    Planes p;
    // misaligned + same buffer, on one output: misaligned
    p = all_far(); p.accum = f4(kFar + 8); p.moments = f4(kFar + 8);
    CHECK(full(p) == kMisaligned);
    // ... the pair first, the misaligned output behind it: same buffer
    p = all_far(); p.moments = p.accum; p.normal_depth = f4(kFar + 0x4000 + 8);
    CHECK(full(p) == kSame);
    // ... the misaligned output first, the pair behind it: misaligned
    p = all_far(); p.accum = f4(kFar + 8); p.normal_depth = p.albedo;
    CHECK(full(p) == kMisaligned);
    // misaligned + range, on one output: misaligned
    p = all_far(); p.moments = f4(kBase + 8);
    CHECK(full(p) == kMisaligned);
    // ... an aligned output in the range first, a misaligned one behind it: the range
    p = all_far(); p.accum = f4(kBase); p.albedo = f4(kFar + 0x3000 + 4);
    CHECK(full(p) == kRangeMsg);
    // ... the misaligned output first: misaligned
    p = all_far(); p.accum = f4(kFar + 4); p.albedo = f4(kBase);
    CHECK(full(p) == kMisaligned);
    // same buffer + range, the pair inside the range: same buffer
    p = all_far(); p.accum = f4(kBase + 32); p.normal_depth = f4(kBase + 32);
    CHECK(full(p) == kSame);
    // ... an output in the range first, the pair behind it: the range
    p = all_far(); p.accum = f4(kBase + 32); p.normal_depth = p.albedo;
    CHECK(full(p) == kRangeMsg);
    // ... the pair first, an output in the range behind it: same buffer
    p = all_far(); p.moments = p.accum; p.normal_depth = f4(kBase + 32);
    CHECK(full(p) == kSame);
    // all three on one output
    p = all_far(); p.accum = f4(kBase + 8); p.moments = f4(kBase + 8);
    CHECK(full(p) == kMisaligned);
}

// The range [kBase, kBase + kRange) against an output's [at, at + npix * elem),
// byte by byte at both ends (alignment not asked, so every address is allowed).
void test_range_ends()
{
    auto one = [](Planes p) { return check_planes("E", p, kPix, &kForbidden, true, false).code; };
    const uintptr_t f_bytes = kPix * 16, b_bytes = kPix * 4;
    // a float4 output: ends just before the range / its last byte is the range's first
    CHECK(one(Planes{f4(kBase - f_bytes)}) == PTG_OK);
    CHECK(one(Planes{f4(kBase - f_bytes + 1)}) == PTG_E_INVALID);
    // starts at the range's first byte, at its last byte, just behind it
    CHECK(one(Planes{f4(kBase)}) == PTG_E_INVALID);
    CHECK(one(Planes{f4(kBase + kRange - 1)}) == PTG_E_INVALID);
    CHECK(one(Planes{f4(kBase + kRange)}) == PTG_OK);
    // the same for every float4 output
    for(uintptr_t at: {kBase - f_bytes + 1, kBase + kRange - 1})
    {
        CHECK(one(Planes{nullptr, nullptr, f4(at)}) == PTG_E_INVALID);
        CHECK(one(Planes{nullptr, nullptr, nullptr, f4(at)}) == PTG_E_INVALID);
        CHECK(one(Planes{nullptr, nullptr, nullptr, nullptr, f4(at)}) == PTG_E_INVALID);
    }
    // bgra is 4 bytes a pixel: it fits where a float4 output does not
    CHECK(one(Planes{nullptr, u4(kBase - b_bytes)}) == PTG_OK);
    CHECK(one(Planes{f4(kBase - b_bytes)}) == PTG_E_INVALID);
    CHECK(one(Planes{nullptr, u4(kBase - b_bytes + 1)}) == PTG_E_INVALID);
    CHECK(one(Planes{nullptr, u4(kBase + kRange - 1)}) == PTG_E_INVALID);
    CHECK(one(Planes{nullptr, u4(kBase + kRange)}) == PTG_OK);
    // an output that holds the whole range
    CHECK(check_planes("E", Planes{f4(kBase - 16)}, 1024, &kForbidden, true, false).code == PTG_E_INVALID);
    // an empty range forbids nothing; an output at the top of the address space does not wrap
    const ForbiddenRange empty{reinterpret_cast<const void*>(kBase), 0, "x"};
    CHECK(check_planes("E", Planes{f4(kBase)}, kPix, &empty, true, false).code == PTG_OK);
    CHECK(one(Planes{f4(~uintptr_t(0) - 15)}) == PTG_OK);
    const ForbiddenRange top{reinterpret_cast<const void*>(~uintptr_t(0) - 255), 256, "x"};
    CHECK(check_planes("E", Planes{f4(kFar)}, kPix, &top, true, false).code == PTG_OK);
    CHECK(check_planes("E", Planes{f4(~uintptr_t(0) - 15)}, 1, &top, true, false).code == PTG_E_INVALID);
}

// bgra is aligned to its 4-byte pixel, the float4 outputs to 16 bytes
void test_alignment_elements()
{
    auto one = [](Planes p) { return check_planes("E", p, kPix, nullptr, true, true).code; };
    for(uintptr_t off: {4u, 8u, 12u})
    {
        CHECK(one(Planes{nullptr, u4(kFar + off)}) == PTG_OK);
        CHECK(one(Planes{f4(kFar + off)}) == PTG_E_INVALID);
        CHECK(one(Planes{nullptr, nullptr, f4(kFar + off)}) == PTG_E_INVALID);
        CHECK(one(Planes{nullptr, nullptr, nullptr, f4(kFar + off)}) == PTG_E_INVALID);
        CHECK(one(Planes{nullptr, nullptr, nullptr, nullptr, f4(kFar + off)}) == PTG_E_INVALID);
    }
    for(uintptr_t off: {1u, 2u, 3u, 5u}) CHECK(one(Planes{nullptr, u4(kFar + off)}) == PTG_E_INVALID);
}

// include/ptg.h: S = pack_tiles * tile_w * tile_h slots; accum at 0, moments at
// 16 S, albedo at 32 S, normal_depth at 48 S, bgra at 64 S; 68 S bytes rounded
// up to a multiple of 256.
void test_pack_carving()
{
    const uint32_t tiles[3][2] = {{1, 1}, {8, 8}, {13, 7}};
    for(const auto& t: tiles)
        for(uint32_t pack_tiles: {1u, 3u, 5u})
        {
            const uint64_t S = uint64_t(pack_tiles) * t[0] * t[1];
            CHECK(tile_pack_slots(t[0], t[1], pack_tiles) == S);
            const size_t bytes = tile_pack_bytes(S);
            CHECK(bytes % 256 == 0 && bytes >= 68 * S && bytes < 68 * S + 256);
#ifndef PLANE_SET_NO_LIB
            CHECK(ptg_tile_pack_bytes(t[0], t[1], pack_tiles) == bytes);
#endif
            char* base = static_cast<char*>(aligned_alloc(256, bytes));
            CHECK(base != nullptr);
            if(!base) continue;
            const Planes pl = pack_planes(base, size_t(S));
            CHECK(reinterpret_cast<char*>(pl.accum) == base);
            CHECK(reinterpret_cast<char*>(pl.moments) == base + 16 * S);
            CHECK(reinterpret_cast<char*>(pl.albedo) == base + 32 * S);
            CHECK(reinterpret_cast<char*>(pl.normal_depth) == base + 48 * S);
            CHECK(reinterpret_cast<char*>(pl.bgra) == base + 64 * S);
            // the last plane ends inside the pack
            CHECK(reinterpret_cast<char*>(pl.bgra) + 4 * S <= base + bytes);
            // a pack's planes pass the check every entry makes, and lie inside the pack
            CHECK(check_planes("E", pl, S, nullptr, true, true).code == PTG_OK);
            const ForbiddenRange self{base, bytes, "overlaps the packs"};
            CHECK(check_planes("E", pl, S, &self, true, true).code == PTG_E_INVALID);
            free(base);
        }
    // ptg.h's example: one 5 x 3 tile is 1020 bytes of planes, 1024 with the padding
    CHECK(tile_pack_bytes(tile_pack_slots(5, 3, 1)) == 1024);
    // a zero dimension: no slot and no byte
    CHECK(tile_pack_slots(0, 8, 1) == 0 && tile_pack_slots(8, 0, 1) == 0 && tile_pack_slots(8, 8, 0) == 0);
    CHECK(tile_pack_bytes(0) == 0);
    // the slots stay below 2^31: refused at 2^31 through the tile and through the count
    CHECK(tile_pack_slots(65536, 32768, 1) == 0);
    CHECK(tile_pack_slots(32768, 32768, 2) == 0);
    CHECK(tile_pack_slots(32768, 32768, 1) == (1ull << 30));
    CHECK(tile_pack_slots(2147483647u, 1, 1) == 2147483647ull);
    CHECK(tile_pack_slots(1, 1, 2147483648u) == 0);
    CHECK(tile_pack_slots(1, 1, 2147483647u) == 2147483647ull);
    CHECK(tile_pack_slots(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu) == 0);
    CHECK(tile_pack_bytes(2147483647ull) == ((68ull * 2147483647ull + 255) & ~255ull));
#ifndef PLANE_SET_NO_LIB
    CHECK(ptg_tile_pack_bytes(65536, 32768, 1) == 0 && ptg_tile_pack_bytes(32768, 32768, 2) == 0);
    CHECK(ptg_tile_pack_bytes(0, 8, 1) == 0 && ptg_tile_pack_bytes(8, 8, 0) == 0);
    CHECK(ptg_tile_pack_bytes(2147483647u, 1, 1) == ((68ull * 2147483647ull + 255) & ~255ull));
#endif
}

} // namespace

int main()
{
    test_rules_alone();
    test_rule_pairs();
    test_range_ends();
    test_alignment_elements();
    test_pack_carving();
    if(g_failed)
    {
        printf("plane_set_test: %d checks FAILED\n", g_failed);
        return 1;
    }
    printf("plane_set_test: all passed\n");
    return 0;
}
