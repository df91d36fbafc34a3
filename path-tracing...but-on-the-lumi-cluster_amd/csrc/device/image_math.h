// Device functions on finished colours and luminance moments, each defined
// once for the two units that use them: the render unit's folds
// (pt_kernels.hip: k_accumulate, k_fold_features, k_ad_fold, k_resolve,
// ad_noisy) and the image-space filters (image_ops.hip).  Only ref_math.h and
// the plane set (host/planes.h) are needed: no ray, no scene, no path state.
//
//   finite3()                        every component finite
//   aces(), srgb(), tonemap()        tonemap_pixel (path_tracer.hh:753-771)
//   lum709()                         Rec. 709 luminance
//   var_of_mean(), moments_of()      the luminance moments' closing arithmetic
//   as_f4(), as_uc4()                ptg.h's pixel types as HIP's vector types
//   close_radiance(), close_moments(), close_feature()
//                                    a pixel's running sums closed into its planes
#pragma once
#include "ref_math.h"
#include "host/planes.h"

namespace ptg {
namespace dm {

PTG_D bool finite3(f3 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }

// tonemap_pixel (:753-771): ACES fit, sRGB curve, clamp, BGRA
PTG_D float aces(float c) { return (c * (2.51f * c + 0.03f)) / (c * (2.43f * c + 0.59f) + 0.14f); }
PTG_D float srgb(float c)
{
    return c < 0.0031308f ? c * 12.92f
                          : (float)(dpow((double)c, (double)(1.0f / 2.4f)) * (double)1.055f - (double)0.055f);
}
PTG_D uchar4 tonemap(f3 c)
{
    const float r = clampf(srgb(aces(c.x)), 0.0f, 1.0f);
    const float g = clampf(srgb(aces(c.y)), 0.0f, 1.0f);
    const float b = clampf(srgb(aces(c.z)), 0.0f, 1.0f);
    return make_uchar4((unsigned char)roundf(b * 255.0f), (unsigned char)roundf(g * 255.0f),
                       (unsigned char)roundf(r * 255.0f), 255);
}

// Rec. 709 luminance of the moments and of the guided denoiser: three
// products, two sums, each one float32 rounding
__device__ __forceinline__ float lum709(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// the variance of the mean of n samples with the moments (m1, m2); a NaN gives 0
__device__ __forceinline__ float var_of_mean(float m1, float m2, float n)
{
    const float d = m2 - m1 * m1;
    const float var = d > 0.0f ? d : 0.0f;
    return n >= 2.0f ? var / (n - 1.0f) : 0.0f;
}
// the sums (s1, s2) of n > 0 finite samples -> (m1, m2, variance of the mean, n)
__device__ __forceinline__ float4 moments_of(float s1, float s2, uint32_t n)
{
    const float nf = (float)n;
    const float m1 = s1 / nf, m2 = s2 / nf;
    return make_float4(m1, m2, var_of_mean(m1, m2, nf), nf);
}

// ptg.h's pixel types (the plane set's) as the HIP vector types of the same layout
__host__ __device__ __forceinline__ float4* as_f4(ptg_float4* p) { return reinterpret_cast<float4*>(p); }
__host__ __device__ __forceinline__ uchar4* as_uc4(ptg_uchar4* p) { return reinterpret_cast<uchar4*>(p); }

// The closing arithmetic: pixel p's running sums (Sums) into its planes
// (Planes).  Its one home: the last chunk of the folds (k_accumulate,
// k_fold_features: div = spp) and the deferred resolve (k_resolve: spp, the
// samples taken, or the pixel's own count) all call these, so their bits are
// the same by construction.  Every division is one correctly rounded float32
// division of the sum by `div`: no reciprocal, no reordering.
//
// The radiance sum / div into out.accum and its tonemap into out.bgra, each
// where the output is given.  `inside` false (a tile map's queue pixel outside
// the image): zeros in both.
PTG_D void close_radiance(float sx, float sy, float sz, float div, bool inside, const Planes& out, uint32_t p)
{
    const float ax = sx / div, ay = sy / div, az = sz / div;
    if(out.accum) as_f4(out.accum)[p] = inside ? make_float4(ax, ay, az, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    if(out.bgra) as_uc4(out.bgra)[p] = inside ? tonemap(V3(ax, ay, az)) : make_uchar4(0, 0, 0, 0);
}
// The luminance sums (s1, s2) of n finite samples into out.moments, which the
// caller knows to be given; zeros outside the image and where n = 0.
PTG_D void close_moments(float s1, float s2, uint32_t n, bool inside, const Planes& out, uint32_t p)
{
    as_f4(out.moments)[p] = inside && n > 0 ? moments_of(s1, s2, n) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// One feature plane's four sums / div into `plane` (out.albedo or
// out.normal_depth, given).  Whether a pixel outside the image is written at
// all is the caller's: the folds skip it, as k_features does.
PTG_D void close_feature(float4 sum, float div, ptg_float4* plane, uint32_t p)
{
    as_f4(plane)[p] = make_float4(sum.x / div, sum.y / div, sum.z / div, sum.w / div);
}

} // namespace dm
} // namespace ptg
