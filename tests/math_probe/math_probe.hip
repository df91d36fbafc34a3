// The rounding certificates (ref_math.h: float_certain, the seven MathFast
// wrappers) and the glibc restatement (glibc_math.h) behind C entry points
// over device arrays, so tests/test_gpu_math_probe.py can drive them with
// constructed inputs and compare them with the host's libm (math_ref.cpp,
// the same library).  Test infrastructure; nothing here is linked into the
// product.  Every entry point returns the HIP status.
//
// A wrapper's arguments travel as doubles, args[k * n + i] being argument k
// of case i in the wrapper's own order (a float argument is widened, which is
// exact, and narrowed again on the device):
//   acc_exp(acc, x)   exp_times(x, s)   add_mul_pow(a, b, x, y)
//   div_mul_pow(a, b, x, y)   times_cos(s, phi)   times_sin(s, phi)
//   times_one_minus_div_pow(r, g, x, y)
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device/path_tracer.h"

using namespace ptg::dm;
namespace gl = ptg::glibc;

namespace {

constexpr uint32_t kArgs = 4;

// y is a literal at the path's call sites (pow_fast's comparison folds): the
// path's exponent of each wrapper takes the literal here too
template<class MP>
__device__ float call_site(int site, const double* __restrict__ a, uint32_t n, uint32_t i, MP& mp)
{
    const double a0 = a[i], a1 = a[n + i], a2 = a[2 * n + i], a3 = a[3 * n + i];
    switch(site)
    {
    case CS_ACC_EXP: return acc_exp((float)a0, a1, mp);
    case CS_EXP_TIMES: return exp_times(a0, (float)a1, mp);
    case CS_ADD_MUL_POW:
        return a3 == 5.0 ? add_mul_pow((float)a0, (float)a1, a2, 5.0, mp) : add_mul_pow((float)a0, (float)a1, a2, a3, mp);
    case CS_DIV_MUL_POW: return a3 == 1.5 ? div_mul_pow(a0, a1, a2, 1.5, mp) : div_mul_pow(a0, a1, a2, a3, mp);
    case CS_TIMES_COS: return times_cos((float)a0, a1, mp);
    case CS_TIMES_SIN: return times_sin((float)a0, a1, mp);
    case CS_TIMES_ONE_MINUS_DIV_POW:
        return a3 == 0.25 ? times_one_minus_div_pow((float)a0, a1, a2, 0.25, mp)
                          : times_one_minus_div_pow((float)a0, a1, a2, a3, mp);
    }
    return 0.0f;
}

__global__ void k_float_certain(uint32_t n, const uint64_t* __restrict__ v, const uint32_t* __restrict__ margin,
                                uint8_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    out[i] = float_certain(gl::asd(v[i]), margin[i]) ? 1 : 0;
}

__global__ void k_wrapper(int site, uint32_t n, const double* __restrict__ args, uint32_t* __restrict__ fast_bits,
                          uint32_t* __restrict__ fail_mask, uint32_t* __restrict__ exact_bits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    MathFast mf;
    fast_bits[i] = __float_as_uint(call_site(site, args, n, i, mf));
    fail_mask[i] = mf.fail_mask;
    MathExact mx;
    exact_bits[i] = __float_as_uint(call_site(site, args, n, i, mx));
}

// MathExactLds as the sky kernel sets it up: the block copies exp's table to
// LDS and synchronises before any thread uses it (or returns)
__global__ void k_wrapper_lds(int site, uint32_t n, const double* __restrict__ args, uint32_t* __restrict__ lds_bits)
{
    __shared__ gl::u2v exp_tab[gl::kExpTabEntries];
    gl::exp_table_to_lds((gl::lds_u2v_t*)exp_tab);   // C cast: generic -> LDS address space
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    MathExactLds mp;
    mp.xt = gl::ExpTabLds{(const gl::lds_u2v_t*)exp_tab};
    lds_bits[i] = __float_as_uint(call_site(site, args, n, i, mp));
}

enum LibFn { LF_EXP, LF_POW, LF_SIN, LF_COS, LF_POW5, LF_POW_QUARTER, LF_COUNT };

__global__ void k_lib(int fn, uint32_t n, const uint64_t* __restrict__ x, double y, uint64_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    const double v = gl::asd(x[i]);
    double r = 0.0;
    switch(fn)
    {
    case LF_EXP: r = dexp(v); break;
    case LF_POW: r = dpow(v, y); break;
    case LF_SIN: r = dsin(v); break;
    case LF_COS: r = dcos(v); break;
    case LF_POW5: r = pow5_d(v); break;
    case LF_POW_QUARTER: r = pow_quarter_d(v); break;
    }
    out[i] = gl::asu(r);
}

int finish()
{
    hipError_t e = hipGetLastError();
    if(e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}

constexpr uint32_t kThreads = 256;
uint32_t blocks(uint32_t n, uint32_t block) { return (n + block - 1) / block; }

} // namespace

extern "C" {

uint32_t math_probe_cert_ulps() { return kCertUlps; }
uint32_t math_probe_max_lib_dist() { return kMaxLibDist; }
uint32_t math_probe_args() { return kArgs; }

int math_probe_float_certain(uint32_t n, const uint64_t* v, const uint32_t* margin, uint8_t* out)
{
    if(n == 0) return 0;
    hipLaunchKernelGGL(k_float_certain, dim3(blocks(n, kThreads)), dim3(kThreads), 0, nullptr, n, v, margin, out);
    return finish();
}

int math_probe_wrapper(int site, uint32_t n, const double* args, uint32_t* fast_bits, uint32_t* fail_mask,
                       uint32_t* exact_bits)
{
    if(site < 0 || site >= CS_COUNT) return (int)hipErrorInvalidValue;
    if(n == 0) return 0;
    hipLaunchKernelGGL(k_wrapper, dim3(blocks(n, kThreads)), dim3(kThreads), 0, nullptr, site, n, args, fast_bits, fail_mask,
                       exact_bits);
    return finish();
}

int math_probe_wrapper_lds(int site, uint32_t block, uint32_t n, const double* args, uint32_t* lds_bits)
{
    if(site < 0 || site >= CS_COUNT || (block != 64 && block != 256)) return (int)hipErrorInvalidValue;
    if(n == 0) return 0;
    hipLaunchKernelGGL(k_wrapper_lds, dim3(blocks(n, block)), dim3(block), 0, nullptr, site, n, args, lds_bits);
    return finish();
}

int math_probe_lib(int fn, uint32_t n, const uint64_t* x, double y, uint64_t* out)
{
    if(fn < 0 || fn >= LF_COUNT) return (int)hipErrorInvalidValue;
    if(n == 0) return 0;
    hipLaunchKernelGGL(k_lib, dim3(blocks(n, kThreads)), dim3(kThreads), 0, nullptr, fn, n, x, y, out);
    return finish();
}

} // extern "C"
