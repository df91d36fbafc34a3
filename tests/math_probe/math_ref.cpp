// The host reference of every entry of math_probe.hip: the reference
// renderer's plain expression with this host's libm (as the !MP::kFast
// branches of ref_math.h and oracle/pt_oracle.c state it).  Compiled with
// -fno-builtin -ffp-contract=off -fno-fast-math (Makefile), so every call
// reaches libm and no operation is fused.  Host code only.
//
// Argument layout as in math_probe.hip: args[k * n + i] is argument k of
// case i, a float argument widened to double.
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace {

enum Site { ACC_EXP, EXP_TIMES, ADD_MUL_POW, DIV_MUL_POW, TIMES_COS, TIMES_SIN, TIMES_ONE_MINUS_DIV_POW, SITES };
enum LibFn { LF_EXP, LF_POW, LF_SIN, LF_COS, LF_POW5, LF_POW_QUARTER, LF_COUNT };

uint64_t dbits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
double dfrom(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float ffrom(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// the double the reference rounds to float; q and w of the regularisation
// term on the side (times_one_minus_div_pow only)
double value(int site, double a0, double a1, double a2, double a3, double* q, double* w)
{
    switch(site)
    {
    case ACC_EXP: return (double)(float)a0 + exp(a1);
    case EXP_TIMES: return exp(a0) * (double)(float)a1;
    case ADD_MUL_POW: return (double)(float)a0 + (double)(float)a1 * pow(a2, a3);
    case DIV_MUL_POW: return a0 / (a1 * pow(a2, a3));
    case TIMES_COS: return (double)(float)a0 * cos(a1);
    case TIMES_SIN: return (double)(float)a0 * sin(a1);
    case TIMES_ONE_MINUS_DIV_POW:
    {
        const double qq = a1 / pow(a2, a3);
        const double ww = fmax(1 - qq, 0.0);
        if(q) *q = qq;
        if(w) *w = ww;
        return (double)(float)a0 * ww;
    }
    }
    return 0.0;
}

// the Mie phase's arguments of div_mul_pow from mu, in the path's float arithmetic
void mie_args(float mu, double* a, double* b, double* x)
{
    const float g = 0.80f;
    const float pi = (float)3.14159265358979323846;
    *a = (double)(3.0f / (8.0f * pi) * (1.0f - g * g) * (1.0f + mu * mu));
    *b = (double)(2.0f + g * g);
    *x = (double)(1.0f + g * g - 2.0f * g * mu);
}

} // namespace

extern "C" {

// out_f32[i]: the reference's float bits; out_v[i]: the double it rounds;
// out_qw (times_one_minus_div_pow, may be null): q at [i], w at [n + i]
void math_ref_wrapper(int site, uint32_t n, const double* args, uint32_t* out_f32, uint64_t* out_v, double* out_qw)
{
    for(uint32_t i = 0; i < n; ++i)
    {
        double q = 0, w = 0;
        const double v = value(site, args[i], args[n + i], args[2 * n + i], args[3 * n + i], &q, &w);
        if(out_f32) out_f32[i] = fbits((float)v);
        if(out_v) out_v[i] = dbits(v);
        if(out_qw && site == TIMES_ONE_MINUS_DIV_POW)
        {
            out_qw[i] = q;
            out_qw[n + i] = w;
        }
    }
}

void math_ref_lib(int fn, uint32_t n, const uint64_t* x, double y, uint64_t* out)
{
    for(uint32_t i = 0; i < n; ++i)
    {
        const double v = dfrom(x[i]);
        double r = 0.0;
        switch(fn)
        {
        case LF_EXP: r = exp(v); break;
        case LF_POW: r = pow(v, y); break;
        case LF_SIN: r = sin(v); break;
        case LF_COS: r = cos(v); break;
        case LF_POW5: r = pow(v, 5.0); break;
        case LF_POW_QUARTER: r = pow(v, 0.25); break;
        }
        out[i] = dbits(r);
    }
}

// args (4 columns of n): a, b, x, y = 1.5 of the Mie phase for each mu
void math_ref_mie_args(uint32_t n, const float* mu, double* args)
{
    for(uint32_t i = 0; i < n; ++i)
    {
        mie_args(mu[i], &args[i], &args[n + i], &args[2 * n + i]);
        args[3 * n + i] = 1.5;
    }
}

// Near-midpoint search (tests/golden/make_cert_golden.py): with the other
// arguments fixed (fixed[0..3]), argument `scan_arg` runs over the floats
// base_bits + m, m in [0, count).  A case is kept when the reference
// double lies in float's normal range within max_dist double ulps of a float
// rounding midpoint.  Returns the number of hits (at most max_hits are
// stored): the scanned float's bits and the distance.
uint32_t math_ref_scan(int site, const double* fixed, int scan_arg, uint32_t base_bits, uint32_t count, uint32_t max_dist,
                       uint32_t max_hits, uint32_t* hit_bits, uint32_t* hit_dist)
{
    uint32_t hits = 0;
    double a[4] = {fixed[0], fixed[1], fixed[2], fixed[3]};
    for(uint32_t m = 0; m < count; ++m)
    {
        const float f = ffrom(base_bits + m);
        a[scan_arg] = (double)f;
        const uint64_t u = dbits(value(site, a[0], a[1], a[2], a[3], 0, 0));
        const uint32_t e = (uint32_t)(u >> 52) & 0x7ffu;
        if(e - (1023u - 126u) > 253u) continue;
        const uint32_t low = (uint32_t)u & 0x1fffffffu;
        const uint32_t d = low > 0x10000000u ? low - 0x10000000u : 0x10000000u - low;
        if(d > max_dist) continue;
        if(hits < max_hits)
        {
            hit_bits[hits] = base_bits + m;
            hit_dist[hits] = d;
        }
        ++hits;
    }
    return hits;
}

} // extern "C"
