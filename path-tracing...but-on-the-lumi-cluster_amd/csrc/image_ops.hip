// The image-space filters of the C ABI (include/ptg.h): kernels over finished
// per-pixel images, and their entry points.  Nothing here traces a ray or
// reads the scene, a path queue or a render job: the unit includes ref_math.h
// and image_math.h, and neither the walker nor the wavefront pipeline.
//
//   k_tonemap       tonemap_pixel per pixel (ptg_tonemap, ptg_tonemap_device)
//   k_dn_demodulate<GUIDED>, k_dn_atrous<STEP>, k_dn_remodulate
//                   the a-trous denoisers: STEP is DenoiseStep (fixed sigmas)
//                   or DenoiseGuidedStep (variance-guided)
//   k_temporal_accumulate<CLAMPED>  last frame's radiance and moments,
//                   reprojected and blended with this frame's by sample count;
//                   <true> through a list of cameras, the history clamped to
//                   the frame's local colour range
//
// No fallback path exists: every entry point fails loudly (negative code +
// ptg_last_error) when HIP or the device is unavailable.
#include "runtime.h"
#include "device/ref_math.h"
#include "device/image_math.h"
#include <cmath>
#include <utility>

using namespace ptg;
using namespace ptg::dm;

namespace {

// ---------------------------------------------------------------- kernels --

__global__ void k_tonemap(uint32_t n, const float4* __restrict__ in, uchar4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) out[i] = tonemap(V3(in[i].x, in[i].y, in[i].z));
}

// max(albedo, floor) of the denoiser's (de)modulation; a NaN albedo stays NaN
__device__ __forceinline__ float dn_floor(float a, float fl) { return (a > fl || a != a) ? a : fl; }

// a variance the guided denoiser may use: >= 0 and finite, else 0
__device__ __forceinline__ float dn_var_ok(float v) { return (v >= 0.0f && __builtin_isfinite(v)) ? v : 0.0f; }

// I0 = radiance / max(albedo, floor) per channel.  GUIDED (ptg_denoise_guided):
// the w lane is V0, the variance of the pixel's mean luminance (moments.z) /
// lum(max(albedo, floor))^2; else it is 0 and moments is not read.
template<bool GUIDED>
__global__ __launch_bounds__(kBlock) void k_dn_demodulate(uint32_t n, float fl, const float4* __restrict__ radiance,
                                                          const float4* __restrict__ albedo,
                                                          const float4* __restrict__ moments, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    const float4 r = radiance[i], a = albedo[i];
    const float mx = dn_floor(a.x, fl), my = dn_floor(a.y, fl), mz = dn_floor(a.z, fl);
    float4 o = make_float4(r.x / mx, r.y / my, r.z / mz, 0.0f);
    if constexpr(GUIDED)
    {
        const float v = dn_var_ok(moments[i].z);
        const float ml = lum709(mx, my, mz);
        o.w = dn_var_ok(v / (ml * ml));
    }
    out[i] = o;
}

// One iteration's arguments: the fixed filter's colour range (ptg_denoise) or
// the guided filter's luminance range (ptg_denoise_guided), and what they share
struct DenoiseStep {
    static constexpr bool guided = false;
    uint32_t w, h, step;
    float var_color, var_albedo, var_normal, var_depth;   // sigma * sigma of this iteration
};
struct DenoiseGuidedStep {
    static constexpr bool guided = true;
    uint32_t w, h, step;
    float sigma_luminance, variance_floor;
    float var_albedo, var_normal, var_depth;              // sigma * sigma
};

// One edge-avoiding a-trous iteration, one work-item per pixel: 5 x 5 taps
// `step` pixels apart, dy outer and dx inner, every operation one float32
// rounding in the order DESIGN.md gives; the weight's exp is glibc's.
// The fixed filter (STEP = DenoiseStep) compares colours against var_color.
// The guided one (DenoiseGuidedStep) filters (I.xyz, V): a 3 x 3 prefilter of
// V at distance 1 sets the range of the luminance difference, and the taps
// filter V with the squares of the weights.
template<class STEP>
__global__ __launch_bounds__(kBlock) void k_dn_atrous(STEP a, const float4* __restrict__ I,
                                                      const float4* __restrict__ albedo,
                                                      const float4* __restrict__ normal_depth, float4* __restrict__ out)
{
    constexpr bool GUIDED = STEP::guided;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= a.w * a.h) return;
    const int32_t x = (int32_t)(i % a.w), y = (int32_t)(i / a.w);
    const float4 Ip = I[i], Ap = albedo[i], Np = normal_depth[i];
    float den = 0.0f, lp = 0.0f;
    if constexpr(GUIDED)
    {
        float gs = 0.0f, gn = 0.0f;
        for(int32_t dy = -1; dy <= 1; ++dy)
        {
            const int32_t qy = y + dy;
            if(qy < 0 || qy >= (int32_t)a.h) continue;
            const float ty = dy == 0 ? 0.5f : 0.25f;
            for(int32_t dx = -1; dx <= 1; ++dx)
            {
                const int32_t qx = x + dx;
                if(qx < 0 || qx >= (int32_t)a.w) continue;
                const float tx = dx == 0 ? 0.5f : 0.25f;
                const float4 Iq = I[size_t(qy) * a.w + size_t(qx)];
                if(!finite3(V3(Iq.x, Iq.y, Iq.z))) continue;
                const float gw = ty * tx;
                gs = gs + gw * Iq.w;
                gn = gn + gw;
            }
        }
        const float g = gn > 0.0f ? gs / gn : 0.0f;
        den = a.sigma_luminance * sqrtf(g) + a.variance_floor;
        lp = lum709(Ip.x, Ip.y, Ip.z);
    }
    const bool p_finite = finite3(V3(Ip.x, Ip.y, Ip.z));
    const float zp2 = Np.w * Np.w;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
    for(int32_t dy = -2; dy <= 2; ++dy)
    {
        const int64_t qy = (int64_t)y + (int64_t)dy * a.step;
        if(qy < 0 || qy >= (int64_t)a.h) continue;
        const float hy = dy == 0 ? 0.375f : (dy == -1 || dy == 1) ? 0.25f : 0.0625f;
        for(int32_t dx = -2; dx <= 2; ++dx)
        {
            const int64_t qx = (int64_t)x + (int64_t)dx * a.step;
            if(qx < 0 || qx >= (int64_t)a.w) continue;
            const float hx = dx == 0 ? 0.375f : (dx == -1 || dx == 1) ? 0.25f : 0.0625f;
            const size_t q = size_t(qy) * a.w + size_t(qx);
            const float4 Iq = I[q];
            if(!finite3(V3(Iq.x, Iq.y, Iq.z))) continue;
            const float4 Aq = albedo[q], Nq = normal_depth[q];
            float ec = 0.0f;                                            // the colour or luminance term
            if constexpr(GUIDED)
                ec = p_finite ? fabsf(lp - lum709(Iq.x, Iq.y, Iq.z)) / den : 0.0f;
            else
            {
                float dc = 0.0f;
                if(p_finite)
                {
                    const float cx = Ip.x - Iq.x, cy = Ip.y - Iq.y, cz = Ip.z - Iq.z;
                    dc = (cx * cx + cy * cy) + cz * cz;
                }
                ec = dc / a.var_color;
            }
            const float ax = Ap.x - Aq.x, ay = Ap.y - Aq.y, az = Ap.z - Aq.z, aw = Ap.w - Aq.w;
            const float da = ((ax * ax + ay * ay) + az * az) + aw * aw;
            const float nx = Np.x - Nq.x, ny = Np.y - Nq.y, nz = Np.z - Nq.z;
            const float dn = (nx * nx + ny * ny) + nz * nz;
            const float dz = Np.w - Nq.w;
            const float zq2 = Nq.w * Nq.w;
            const float zmax = (zp2 > zq2 || zp2 != zp2) ? zp2 : zq2;   // a NaN depth stays NaN
            const float dz2 = (dz * dz) / (zmax + 1e-12f);
            const float e = ((ec + da / a.var_albedo) + dn / a.var_normal) + dz2 / a.var_depth;
            if(!__builtin_isfinite(e)) continue;
            const float wgt = (hy * hx) * (float)dexp(-(double)e);
            sw = sw + wgt;
            sx = sx + wgt * Iq.x;
            sy = sy + wgt * Iq.y;
            sz = sz + wgt * Iq.z;
            if constexpr(GUIDED) sv = sv + (wgt * wgt) * Iq.w;
        }
    }
    // the w lane: the guided filter's variance, else 0
    out[i] = sw > 0.0f ? make_float4(sx / sw, sy / sw, sz / sw, GUIDED ? dn_var_ok(sv / (sw * sw)) : 0.0f)
                       : make_float4(Ip.x, Ip.y, Ip.z, GUIDED ? dn_var_ok(Ip.w) : 0.0f);
}

// out = I * max(albedo, floor), w = 0; optionally its tonemap
__global__ __launch_bounds__(kBlock) void k_dn_remodulate(uint32_t n, float fl, const float4* __restrict__ I,
                                                          const float4* __restrict__ albedo, float4* __restrict__ out,
                                                          uchar4* __restrict__ out_bgra)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    const float4 v = I[i], a = albedo[i];
    const f3 c = V3(v.x * dn_floor(a.x, fl), v.y * dn_floor(a.y, fl), v.z * dn_floor(a.z, fl));
    out[i] = make_float4(c.x, c.y, c.z, 0.0f);
    if(out_bgra) out_bgra[i] = tonemap(c);
}

// ---- temporal accumulation (several cameras and the history clamp: 4.17) ----

// The parts of a ptg_camera the reprojection reads.
struct TemporalCam {
    m3 ori;
    f3 pos;
    float aspect, ifl, fd;
};
// k_temporal_accumulate's arguments.  The plain entry reads `cam` and none of
// the clamped entry's fields; the clamped entry reads those and not `cam`.
struct TemporalArgs {
    uint32_t w, h;
    uint32_t has_history;                  // 0: first frame, the hist_* pointers are null
    float max_history, depth_tolerance, normal_tolerance, albedo_tolerance;
    TemporalCam cam, hist;                 // plain: this frame's camera; the history's
    uint32_t n_cams;                       // clamped: this frame's cameras, in the context's buffer
    uint32_t clamp_radius;                 // clamped: 0: no clamp
    float clamp_sigma, clipped_history;    // clamped
};

// Steps 2-4 of the definition for one camera: the first-hit point of pixel
// (x, y), from its centre ray through `cam` and the mean depth z, is
// projected into `hist`; the four bilinear taps around it that show the same
// surface (depth, normal, albedo) add into the seven running sums.  A camera
// that fails a test adds nothing.
struct TemporalSums {
    float sw = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f, s1 = 0.0f, s2 = 0.0f, sn = 0.0f;
};
__device__ __forceinline__ void tp_gather(TemporalSums& s, uint32_t w, uint32_t h, float depth_tolerance,
                                          float normal_tolerance, float albedo_tolerance, const TemporalCam& cam,
                                          const TemporalCam& hist, uint32_t x, uint32_t y, float z, const float4& A,
                                          const float4& G, const float4* __restrict__ hist_radiance,
                                          const float4* __restrict__ hist_moments, const float4* __restrict__ hist_albedo,
                                          const float4* __restrict__ hist_normal_depth)
{
    const float uvx = (((float)x + 0.5f) / (float)w * 2.0f - 1.0f) * cam.aspect;
    const float uvy = -(((float)y + 0.5f) / (float)h * 2.0f - 1.0f);
    const f3 d = normalize(V3(uvx * cam.ifl * cam.fd, uvy * cam.ifl * cam.fd, -1.0f * cam.fd));
    const f3 dir = mul_m3v3(cam.ori, d);
    const f3 P = cam.pos + dir * z;
    const f3 q = P - hist.pos;
    const f3 l = mul_v3m3(q, hist.ori);
    if(l.z < 0.0f)
    {
        const float t = -l.z;
        const float sx = (l.x / t) / hist.ifl / hist.aspect;
        const float sy = -((l.y / t) / hist.ifl);
        const float fx = (sx + 1.0f) * 0.5f * (float)w - 0.5f;
        const float fy = (sy + 1.0f) * 0.5f * (float)h - 0.5f;
        const float ze = fsqrt((q.x * q.x + q.y * q.y) + q.z * q.z);
        if(__builtin_isfinite(fx) && __builtin_isfinite(fy))
        {
            const float ix = floorf(fx), iy = floorf(fy);
            const float tx = fx - ix, ty = fy - iy;
            const float xmax = (float)(w - 1u), ymax = (float)(h - 1u);
#pragma unroll
            for(int b = 0; b < 2; ++b)
            {
                const float Y = iy + (float)b;
                const float wy = b ? ty : 1.0f - ty;
#pragma unroll
                for(int c = 0; c < 2; ++c)
                {
                    const float X = ix + (float)c;
                    const float bw = (c ? tx : 1.0f - tx) * wy;
                    // inside on the floats; an integer only after that
                    if(!(X >= 0.0f && X <= xmax && Y >= 0.0f && Y <= ymax)) continue;
                    const size_t t4 = size_t((uint32_t)Y) * w + size_t((uint32_t)X);
                    const float4 HA = hist_albedo[t4];
                    if(!(HA.w > 0.0f)) continue;
                    const float4 H = hist_radiance[t4];
                    if(!finite3(V3(H.x, H.y, H.z))) continue;
                    const float4 HM = hist_moments[t4];
                    if(!(HM.w > 0.0f)) continue;
                    const float4 HG = hist_normal_depth[t4];
                    const float zh = HG.w / HA.w;
                    const float zm = zh > ze ? zh : ze;
                    if(!(fabsf(zh - ze) <= depth_tolerance * zm)) continue;
                    const float nx = G.x - HG.x, ny = G.y - HG.y, nz = G.z - HG.z;
                    const float dn = (nx * nx + ny * ny) + nz * nz;
                    if(!(dn <= normal_tolerance)) continue;
                    const float ax = A.x - HA.x, ay = A.y - HA.y, az = A.z - HA.z, aw = A.w - HA.w;
                    const float da = ((ax * ax + ay * ay) + az * az) + aw * aw;
                    if(!(da <= albedo_tolerance)) continue;
                    s.sw = s.sw + bw;
                    s.cx = s.cx + bw * H.x;
                    s.cy = s.cy + bw * H.y;
                    s.cz = s.cz + bw * H.z;
                    s.s1 = s.s1 + bw * HM.x;
                    s.s2 = s.s2 + bw * HM.y;
                    s.sn = s.sn + bw * HM.w;
                }
            }
        }
    }
}

// Steps 6-7: the history (hx, hy, hz; h1, h2; hn samples, not yet capped at
// max_history) blended with this frame's R and M by their sample counts, or
// the history alone where this frame brings nothing usable.
__device__ __forceinline__ void tp_blend(float hx, float hy, float hz, float h1, float h2, float hn, float max_history,
                                         const float4& R, const float4& M, float4& oc, float4& om)
{
    const float nh = hn < max_history ? hn : max_history;
    if(finite3(V3(R.x, R.y, R.z)) && M.w > 0.0f)
    {
        const float nt = nh + M.w;
        const float al = M.w / nt;
        oc = make_float4(hx + al * (R.x - hx), hy + al * (R.y - hy), hz + al * (R.z - hz), 0.0f);
        const float m1 = h1 + al * (M.x - h1), m2 = h2 + al * (M.y - h2);
        om = make_float4(m1, m2, var_of_mean(m1, m2, nt), nt);
    }
    else
    {   // nothing usable in this frame: the history alone
        oc = make_float4(hx, hy, hz, 0.0f);
        om = make_float4(h1, h2, var_of_mean(h1, h2, nh), nh);
    }
}

// One work-item per pixel: the pixel's first-hit point, from its centre ray
// through this frame's camera and its mean depth, is projected into `hist`;
// the four bilinear taps around it that show the same surface (depth, normal,
// albedo) give the history's radiance and moments, which are blended with this
// frame's by their sample counts.  Every operation is one float32 rounding in
// the order DESIGN.md gives.  This frame's images are read at the pixel alone
// (the outputs may be the radiance and moments themselves: no __restrict__
// on those four); the history is gathered.
//
// The plain entry (CLAMPED = false) has one camera, a.cam in the kernel
// arguments; `cams` and `flags` are null and never read.  The clamped entry
// has two insertions.  The reprojection runs once per camera of `cams` (a
// wave-uniform loop: the cameras come through scalar loads) into the same
// seven sums, so the history of a motion-blurred pixel is gathered along the
// blur.  With clamp_radius r > 0 the history's colour is then clamped, per
// channel, to mean +- clamp_sigma standard deviations of the finite pixels of
// this frame's (2r + 1)^2 window; a clipped history's first moment follows the
// colour, its second keeps the variance, and its sample count is capped at
// clipped_history.  `radiance` is gathered by the clamp: with r > 0 it is not
// out_radiance (the host refuses that).  flags (optional): bit 0 the pixel
// found history, bit 1 its history was clipped.
template<bool CLAMPED>
__global__ __launch_bounds__(kBlock) void k_temporal_accumulate(
    TemporalArgs a, const float4* radiance, const float4* moments, const float4* __restrict__ albedo,
    const float4* __restrict__ normal_depth, const float4* __restrict__ hist_radiance,
    const float4* __restrict__ hist_moments, const float4* __restrict__ hist_albedo,
    const float4* __restrict__ hist_normal_depth, float4* out_radiance, float4* out_moments, uchar4* __restrict__ out_bgra,
    const TemporalCam* __restrict__ cams, uint8_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= a.w * a.h) return;
    const uint32_t x = i % a.w, y = i / a.w;
    const float4 R = radiance[i], M = moments[i], A = albedo[i], G = normal_depth[i];
    TemporalSums s;
    const float cov = A.w;
    if(a.has_history && cov > 0.0f)
    {
        const float z = G.w / cov;
        auto gather = [&](const TemporalCam& cam) {
            tp_gather(s, a.w, a.h, a.depth_tolerance, a.normal_tolerance, a.albedo_tolerance, cam, a.hist, x, y, z, A, G,
                      hist_radiance, hist_moments, hist_albedo, hist_normal_depth);
        };
        if constexpr(CLAMPED)
            for(uint32_t k = 0; k < a.n_cams; ++k) gather(cams[k]);
        else
            gather(a.cam);   // not a one-trip loop: that compiles to 2 VGPRs more
    }
    float4 oc = make_float4(R.x, R.y, R.z, 0.0f), om = M;      // no history: this frame's bits
    uint32_t fl = 0;
    if(s.sw > 0.0f)
    {
        fl = 1u;
        float hc[3] = {s.cx / s.sw, s.cy / s.sw, s.cz / s.sw};
        float h1 = s.s1 / s.sw, h2 = s.s2 / s.sw, hn = s.sn / s.sw;
        if(CLAMPED && a.clamp_radius)
        {
            const int32_t r = (int32_t)a.clamp_radius;
            int32_t n = 0;
            float su[3] = {0.0f, 0.0f, 0.0f}, sq[3] = {0.0f, 0.0f, 0.0f};
            for(int32_t dy = -r; dy <= r; ++dy)
            {
                const int32_t qy = (int32_t)y + dy;
                if(qy < 0 || qy >= (int32_t)a.h) continue;
                for(int32_t dx = -r; dx <= r; ++dx)
                {
                    const int32_t qx = (int32_t)x + dx;
                    if(qx < 0 || qx >= (int32_t)a.w) continue;
                    const float4 Rq = radiance[size_t(qy) * a.w + size_t(qx)];
                    if(!finite3(V3(Rq.x, Rq.y, Rq.z))) continue;
                    ++n;
                    su[0] = su[0] + Rq.x; sq[0] = sq[0] + Rq.x * Rq.x;
                    su[1] = su[1] + Rq.y; sq[1] = sq[1] + Rq.y * Rq.y;
                    su[2] = su[2] + Rq.z; sq[2] = sq[2] + Rq.z * Rq.z;
                }
            }
            if(n > 0)
            {
                const float nf = (float)n;
                const float l0 = lum709(hc[0], hc[1], hc[2]);
                bool clipped = false;
#pragma unroll
                for(int c = 0; c < 3; ++c)
                {
                    const float mu = su[c] / nf, e2 = sq[c] / nf;
                    const float d = e2 - mu * mu;
                    const float rr = a.clamp_sigma * fsqrt(d > 0.0f ? d : 0.0f);
                    const float lo = mu - rr, hi = mu + rr;
                    // a NaN bound compares false: the value stays
                    if(hc[c] < lo) { hc[c] = lo; clipped = true; }
                    else if(hc[c] > hi) { hc[c] = hi; clipped = true; }
                }
                if(clipped)
                {
                    fl = 3u;
                    const float dl = lum709(hc[0], hc[1], hc[2]) - l0;
                    const float g1 = h1 + dl;
                    h2 = h2 + (g1 * g1 - h1 * h1);
                    h1 = g1;
                    hn = hn < a.clipped_history ? hn : a.clipped_history;
                }
            }
        }
        tp_blend(hc[0], hc[1], hc[2], h1, h2, hn, a.max_history, R, M, oc, om);
    }
    out_radiance[i] = oc;
    out_moments[i] = om;
    if(out_bgra) out_bgra[i] = tonemap(V3(oc.x, oc.y, oc.z));
    if(CLAMPED && flags) flags[i] = (uint8_t)fl;
}

// ------------------------------------------------------------------- host --

// What ptg_denoise and ptg_denoise_guided do once their parameters are
// checked: demodulate into dn_a, `iterations` a-trous passes between dn_a and
// dn_b with the step record step_of(k) (a DenoiseStep or a DenoiseGuidedStep,
// which selects the kernels), remodulate into out_radiance.  `moments` is read
// by the guided demodulate alone.
template<class F>
int denoise_passes(ptg_context* ctx, uint32_t w, uint32_t h, uint32_t iterations, float albedo_floor, F step_of,
                   const ptg_float4* radiance, const ptg_float4* albedo, const ptg_float4* normal_depth,
                   const ptg_float4* moments, ptg_float4* out_radiance, ptg_uchar4* out_bgra)
{
    using Step = decltype(step_of(0u));
    if(uint64_t(w) * h == 0) return PTG_OK;
    if(uint64_t(w) * h >= (1ull << 31)) return fail(PTG_E_RANGE, "image too large");
    const uint32_t n = w * h;
    const float4* rad = reinterpret_cast<const float4*>(radiance);
    const float4* alb = reinterpret_cast<const float4*>(albedo);
    float4* out = reinterpret_cast<float4*>(out_radiance);
    uchar4* bgra = reinterpret_cast<uchar4*>(out_bgra);
    if(iterations == 0)
    {   // the input bits, unchanged
        if(out != rad) PTG_HIP(hipMemcpyAsync(out, rad, size_t(n) * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
        return bgra ? launch_plain(ctx, grid_for(n), k_tonemap, n, out, bgra) : PTG_OK;
    }
    PTG_HIP(ctx->grow(ctx->dn_a, size_t(n) * sizeof(float4)));
    PTG_HIP(ctx->grow(ctx->dn_b, size_t(n) * sizeof(float4)));
    float4* cur = ctx->dn_a.as<float4>();
    float4* nxt = ctx->dn_b.as<float4>();
    if(int r = launch_plain(ctx, grid_for(n), k_dn_demodulate<Step::guided>, n, albedo_floor, rad, alb,
                            reinterpret_cast<const float4*>(moments), cur))
        return r;
    for(uint32_t k = 0; k < iterations; ++k)
    {
        if(int r = launch_plain(ctx, grid_for(n), k_dn_atrous<Step>, step_of(k), cur, alb,
                                reinterpret_cast<const float4*>(normal_depth), nxt))
            return r;
        std::swap(cur, nxt);
    }
    return launch_plain(ctx, grid_for(n), k_dn_remodulate, n, albedo_floor, cur, alb, out, bgra);
}

} // namespace

extern "C" {

int ptg_tonemap_device(ptg_context* ctx, size_t n, const ptg_float4* color, ptg_uchar4* out)
{
    if(int r = bind(ctx)) return r;
    if(!n) return PTG_OK;
    if(!color || !out || n >= (1u << 31)) return fail(PTG_E_INVALID, "ptg_tonemap_device: bad arguments");
    return launch_plain(ctx, grid_for(n), k_tonemap, uint32_t(n), reinterpret_cast<const float4*>(color),
                        reinterpret_cast<uchar4*>(out));
}

int ptg_tonemap(ptg_context* ctx, size_t n, const ptg_float4* color, ptg_uchar4* out)
{
    if(int r = bind(ctx)) return r;
    if(!n) return PTG_OK;
    if(!color || !out || n >= (1u << 30)) return fail(PTG_E_INVALID, "ptg_tonemap: bad arguments");
    PTG_HIP(ctx->grow(ctx->tmp_c, n * sizeof(float4)));
    PTG_HIP(ctx->grow(ctx->tmp_a, n * sizeof(uchar4)));
    PTG_HIP(hipMemcpyAsync(ctx->tmp_c.p, color, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    if(int r = launch_plain(ctx, grid_for(n), k_tonemap, uint32_t(n), ctx->tmp_c.as<float4>(), ctx->tmp_a.as<uchar4>())) return r;
    PTG_HIP(hipMemcpyAsync(out, ctx->tmp_a.p, n * sizeof(uchar4), hipMemcpyDeviceToHost, ctx->stream));
    PTG_HIP(hipStreamSynchronize(ctx->stream));
    return PTG_OK;
}

void ptg_denoise_params_default(ptg_denoise_params* p)
{
    if(!p) return;
    // the best row of tools/denoise_study.py's sweep (profiles/denoise_study/)
    p->iterations = 4;
    p->sigma_color = 2.0f;
    p->sigma_albedo = 0.05f;
    p->sigma_normal = 1.2f;
    p->sigma_depth = 1.0f;
    p->albedo_floor = 0.01f;
}

int ptg_denoise(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_denoise_params* params, const ptg_float4* radiance,
                const ptg_float4* albedo, const ptg_float4* normal_depth, ptg_float4* out_radiance, ptg_uchar4* out_bgra)
{
    if(int r = bind(ctx)) return r;
    if(!params || !radiance || !albedo || !normal_depth || !out_radiance) return fail(PTG_E_INVALID, "ptg_denoise: null argument");
    const ptg_denoise_params P = *params;
    if(P.iterations > 8) return fail(PTG_E_INVALID, "ptg_denoise: more than 8 iterations");
    for(float s: {P.sigma_color, P.sigma_albedo, P.sigma_normal, P.sigma_depth, P.albedo_floor})
        if(!(s > 0.0f) || !std::isfinite(s)) return fail(PTG_E_INVALID, "ptg_denoise: sigmas and albedo_floor must be positive and finite");
    const auto step_of = [&](uint32_t k) {
        DenoiseStep a;
        a.w = w; a.h = h; a.step = 1u << k;
        const float sc = P.sigma_color * (1.0f / float(1u << k));   // sigma_color * 2^-k
        a.var_color = sc * sc;
        a.var_albedo = P.sigma_albedo * P.sigma_albedo;
        a.var_normal = P.sigma_normal * P.sigma_normal;
        a.var_depth = P.sigma_depth * P.sigma_depth;
        return a;
    };
    return denoise_passes(ctx, w, h, P.iterations, P.albedo_floor, step_of, radiance, albedo, normal_depth, nullptr, out_radiance,
                          out_bgra);
}

void ptg_denoise_guided_params_default(ptg_denoise_guided_params* p)
{
    if(!p) return;
    // the best row of tools/denoise_study.py --guided --sweep (profiles/denoise_study/guided_study.json)
    p->iterations = 3;
    p->sigma_luminance = 0.5f;
    p->sigma_albedo = 0.05f;
    p->sigma_normal = 1.2f;
    p->sigma_depth = 1.0f;
    p->albedo_floor = 0.01f;
    p->variance_floor = 1e-2f;
}

int ptg_denoise_guided(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_denoise_guided_params* params,
                       const ptg_float4* radiance, const ptg_float4* albedo, const ptg_float4* normal_depth,
                       const ptg_float4* moments, ptg_float4* out_radiance, ptg_uchar4* out_bgra)
{
    if(int r = bind(ctx)) return r;
    if(!params || !radiance || !albedo || !normal_depth || !moments || !out_radiance)
        return fail(PTG_E_INVALID, "ptg_denoise_guided: null argument");
    const ptg_denoise_guided_params P = *params;
    if(P.iterations > 8) return fail(PTG_E_INVALID, "ptg_denoise_guided: more than 8 iterations");
    for(float s: {P.sigma_luminance, P.sigma_albedo, P.sigma_normal, P.sigma_depth, P.albedo_floor, P.variance_floor})
        if(!(s > 0.0f) || !std::isfinite(s))
            return fail(PTG_E_INVALID, "ptg_denoise_guided: sigmas and floors must be positive and finite");
    const auto step_of = [&](uint32_t k) {
        DenoiseGuidedStep a;
        a.w = w; a.h = h; a.step = 1u << k;
        a.sigma_luminance = P.sigma_luminance;
        a.variance_floor = P.variance_floor;
        a.var_albedo = P.sigma_albedo * P.sigma_albedo;
        a.var_normal = P.sigma_normal * P.sigma_normal;
        a.var_depth = P.sigma_depth * P.sigma_depth;
        return a;
    };
    return denoise_passes(ctx, w, h, P.iterations, P.albedo_floor, step_of, radiance, albedo, normal_depth, moments, out_radiance,
                          out_bgra);
}

void ptg_temporal_params_default(ptg_temporal_params* p)
{
    if(!p) return;
    // the best row of tools/denoise_study.py --temporal --sweep (profiles/denoise_study/temporal_study.json)
    p->max_history = 128.0f;
    p->depth_tolerance = 0.02f;
    p->normal_tolerance = 0.1f;
    p->albedo_tolerance = 0.25f;
}

namespace {

// What ptg_temporal_accumulate and ptg_temporal_accumulate_clamped check alike.
// *given: the history is there (all five) or not (none); *empty: the image has
// no pixel and the call is done.
int temporal_check(const std::string& who, uint32_t w, uint32_t h, const ptg_temporal_params& P, const ptg_camera* hist_cam,
                   const void* const hist[4], const void* out_radiance, const void* out_moments, bool* given_out, bool* empty)
{
    for(float s: {P.max_history, P.depth_tolerance, P.normal_tolerance, P.albedo_tolerance})
        if(!(s > 0.0f) || !std::isfinite(s))
            return fail(PTG_E_INVALID, who + ": max_history and the tolerances must be positive and finite");
    int given = hist_cam ? 1 : 0;
    for(int k = 0; k < 4; ++k) given += hist[k] ? 1 : 0;
    if(given != 0 && given != 5)
        return fail(PTG_E_INVALID, who + ": hist_cam and the four hist_* images are all null or all set");
    if(out_radiance == out_moments) return fail(PTG_E_INVALID, who + ": out_radiance and out_moments are one buffer");
    for(int k = 0; k < 4; ++k)
        if(hist[k] && (hist[k] == out_radiance || hist[k] == out_moments))
            return fail(PTG_E_INVALID, who + ": an output is a hist_* image (the history is gathered from neighbours)");
    *given_out = given != 0;
    *empty = uint64_t(w) * h == 0;
    if(*empty) return PTG_OK;
    // pixel coordinates are compared as floats: exact below 2^24
    if(uint64_t(w) * h >= (1ull << 31) || w > (1u << 24) || h > (1u << 24)) return fail(PTG_E_RANGE, "image too large");
    return PTG_OK;
}

TemporalCam temporal_cam_of(const ptg_camera& c)
{
    TemporalCam t;
    for(int k = 0; k < 3; ++k) t.ori.r[k] = f3{c.orientation.r[k].x, c.orientation.r[k].y, c.orientation.r[k].z};
    t.pos = f3{c.position.x, c.position.y, c.position.z};
    t.aspect = c.aspect_ratio;
    t.ifl = c.inv_focal_length;
    t.fd = c.focal_distance;
    return t;
}

const float4* tp_in(const ptg_float4* p) { return reinterpret_cast<const float4*>(p); }

// What both temporal entries do once they have checked what is their own:
// the common checks, the kernel's arguments, the launch.  `clamped`: the
// clamped entry, with n_cams cameras in `cams` and every field of P; the plain
// entry passes its one camera and P.base alone.
int temporal_run(ptg_context* ctx, const std::string& who, bool clamped, uint32_t w, uint32_t h,
                 const ptg_temporal_clamp_params& P, uint32_t n_cams, const ptg_camera* cams, const ptg_camera* hist_cam,
                 const ptg_float4* radiance, const ptg_float4* moments, const ptg_float4* albedo, const ptg_float4* normal_depth,
                 const ptg_float4* hist_radiance, const ptg_float4* hist_moments, const ptg_float4* hist_albedo,
                 const ptg_float4* hist_normal_depth, ptg_float4* out_radiance, ptg_float4* out_moments, ptg_uchar4* out_bgra,
                 uint8_t* out_flags)
{
    const void* hist[4] = {hist_radiance, hist_moments, hist_albedo, hist_normal_depth};
    bool given = false, empty = false;
    if(int r = temporal_check(who, w, h, P.base, hist_cam, hist, out_radiance, out_moments, &given, &empty)) return r;
    if(empty) return PTG_OK;
    TemporalArgs a;
    a.w = w; a.h = h;
    a.has_history = given ? 1u : 0u;
    a.max_history = P.base.max_history;
    a.depth_tolerance = P.base.depth_tolerance;
    a.normal_tolerance = P.base.normal_tolerance;
    a.albedo_tolerance = P.base.albedo_tolerance;
    a.cam = temporal_cam_of(cams[0]);
    a.hist = temporal_cam_of(given ? *hist_cam : cams[0]);
    a.n_cams = n_cams;
    a.clamp_radius = P.clamp_radius;
    a.clamp_sigma = P.clamp_sigma;
    a.clipped_history = P.clipped_history;
    const TemporalCam* dev_cams = nullptr;
    if(clamped)
    {
        // The cameras go through a pinned staging buffer into the context's
        // device buffer, on the context's stream.  The device buffer is safe
        // against reuse by stream order: the next call's copy runs behind this
        // call's kernel.  The staging buffers alternate, and one is written again
        // only after the copy of two calls ago that read it has completed
        // (HostStage::reserve waits for it).
        PTG_HIP(ctx->grow(ctx->tp_cams, size_t(kTemporalMaxCams) * sizeof(TemporalCam)));
        HostStage& hs = ctx->tp_stage[ctx->tp_stage_next];
        ctx->tp_stage_next ^= 1u;
        PTG_HIP(hs.reserve(size_t(kTemporalMaxCams) * sizeof(TemporalCam)));
        TemporalCam* staged = static_cast<TemporalCam*>(hs.p);
        for(uint32_t k = 0; k < n_cams; ++k) staged[k] = temporal_cam_of(cams[k]);
        PTG_HIP(hipMemcpyAsync(ctx->tp_cams.p, staged, size_t(n_cams) * sizeof(TemporalCam), hipMemcpyHostToDevice, ctx->stream));
        PTG_HIP(hipEventRecord(hs.done, ctx->stream));
        dev_cams = ctx->tp_cams.as<const TemporalCam>();
    }
    return launch_plain(ctx, grid_for(size_t(w) * h), clamped ? k_temporal_accumulate<true> : k_temporal_accumulate<false>, a,
                        tp_in(radiance), tp_in(moments), tp_in(albedo), tp_in(normal_depth), tp_in(hist_radiance),
                        tp_in(hist_moments), tp_in(hist_albedo), tp_in(hist_normal_depth),
                        reinterpret_cast<float4*>(out_radiance), reinterpret_cast<float4*>(out_moments),
                        reinterpret_cast<uchar4*>(out_bgra), dev_cams, out_flags);
}

} // namespace

int ptg_temporal_accumulate(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_temporal_params* params,
                            const ptg_camera* cam, const ptg_camera* hist_cam, const ptg_float4* radiance,
                            const ptg_float4* moments, const ptg_float4* albedo, const ptg_float4* normal_depth,
                            const ptg_float4* hist_radiance, const ptg_float4* hist_moments, const ptg_float4* hist_albedo,
                            const ptg_float4* hist_normal_depth, ptg_float4* out_radiance, ptg_float4* out_moments,
                            ptg_uchar4* out_bgra)
{
    if(int r = bind(ctx)) return r;
    if(!params || !cam || !radiance || !moments || !albedo || !normal_depth || !out_radiance || !out_moments)
        return fail(PTG_E_INVALID, "ptg_temporal_accumulate: null argument");
    ptg_temporal_clamp_params P{};   // no clamp: the kernel's plain instantiation reads the base alone
    P.base = *params;
    return temporal_run(ctx, "ptg_temporal_accumulate", false, w, h, P, 1, cam, hist_cam, radiance, moments, albedo, normal_depth,
                        hist_radiance, hist_moments, hist_albedo, hist_normal_depth, out_radiance, out_moments, out_bgra,
                        nullptr);
}

void ptg_temporal_clamp_params_default(ptg_temporal_clamp_params* p)
{
    if(!p) return;
    ptg_temporal_params_default(&p->base);
    // the best row of tools/denoise_study.py --temporal-clamp --sweep (profiles/denoise_study/temporal_clamp_study.json)
    p->clamp_radius = 1;
    p->clamp_sigma = 2.0f;
    p->clipped_history = 32.0f;
}

int ptg_temporal_accumulate_clamped(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_temporal_clamp_params* params,
                                    uint32_t n_cams, const ptg_camera* cams, const ptg_camera* hist_cam,
                                    const ptg_float4* radiance, const ptg_float4* moments, const ptg_float4* albedo,
                                    const ptg_float4* normal_depth, const ptg_float4* hist_radiance,
                                    const ptg_float4* hist_moments, const ptg_float4* hist_albedo,
                                    const ptg_float4* hist_normal_depth, ptg_float4* out_radiance, ptg_float4* out_moments,
                                    ptg_uchar4* out_bgra, uint8_t* out_flags)
{
    static const std::string who = "ptg_temporal_accumulate_clamped";
    if(int r = bind(ctx)) return r;
    if(!params || !cams || !radiance || !moments || !albedo || !normal_depth || !out_radiance || !out_moments)
        return fail(PTG_E_INVALID, who + ": null argument");
    const ptg_temporal_clamp_params P = *params;
    if(n_cams < 1 || n_cams > kTemporalMaxCams) return fail(PTG_E_INVALID, who + ": 1 .. 512 cameras");
    if(P.clamp_radius > 2) return fail(PTG_E_INVALID, who + ": clamp_radius above 2");
    for(float s: {P.clamp_sigma, P.clipped_history})
        if(!(s > 0.0f) || !std::isfinite(s))
            return fail(PTG_E_INVALID, who + ": clamp_sigma and clipped_history must be positive and finite");
    if(P.clamp_radius > 0 && static_cast<const void*>(out_radiance) == static_cast<const void*>(radiance))
        return fail(PTG_E_INVALID, who + ": out_radiance is radiance, which the clamp gathers from neighbours");
    return temporal_run(ctx, who, true, w, h, P, n_cams, cams, hist_cam, radiance, moments, albedo, normal_depth, hist_radiance,
                        hist_moments, hist_albedo, hist_normal_depth, out_radiance, out_moments, out_bgra, out_flags);
}

} // extern "C"
