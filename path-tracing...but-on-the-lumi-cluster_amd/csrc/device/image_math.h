// Device functions on finished colours and luminance moments, each defined
// once for the two units that use them: the render unit's folds
// (pt_kernels.hip: k_accumulate, k_ad_fold, k_ad_resolve, ad_noisy) and the
// image-space filters (image_ops.hip).  Only ref_math.h is needed: no ray, no
// scene, no path state.
//
//   finite3()                        every component finite
//   aces(), srgb(), tonemap()        tonemap_pixel (path_tracer.hh:753-771)
//   lum709()                         Rec. 709 luminance
//   var_of_mean(), moments_of()      the luminance moments' closing arithmetic
#pragma once
#include "ref_math.h"

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

} // namespace dm
} // namespace ptg
