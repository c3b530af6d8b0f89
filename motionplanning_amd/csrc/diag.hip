// diag.hip — device evaluation of the shared FDLIBM restatement (include/mp_jlmath.h).
#include "../../include/mp_jlmath.h"
#include "runtime.hpp"

namespace {
__global__ void math_kernel(int fn, long long n, const double* x, const double* y, double* out) {
  __shared__ double atab[20];
  __shared__ double arows[4 * MPJ_ATAN_ROWS];
  if (threadIdx.x == 0) mpj_atan_tab_init(atab);
  mpj_atan_rows_fill(arows, threadIdx.x, blockDim.x);
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = x[i];
  double r = 0.0;
  switch (fn) {
    case 0: r = mpj_sin(a); break;
    case 1: r = mpj_cos(a); break;
    case 2: r = mpj_tan(a); break;
    case 3: r = mpj_atan(a); break;
    case 4: r = mpj_atan2(a, y[i]); break;
    case 5: r = mpj_asin(a); break;
    case 6: r = mpj_acos(a); break;
    case 7: r = mpj_exp(a); break;
    case 8: r = mpj_log(a); break;
    case 9: r = mpj_modpi(a); break;
    case 10: r = mpj_sqrt(a); break;
    // branch-free device variants used by the hot kernels (must equal the exact routines)
    case 11: r = mpj_modpi_bl(a); break;
    case 12: r = mpj_atan_bl(a); break;
    case 13: r = mpj_atan_tab(a, atab); break;
    case 14: { double s, c; mpj_sincos_bl(a, &s, &c); r = s; break; }
    case 15: { double s, c; mpj_sincos_bl(a, &s, &c); r = c; break; }
    case 16: r = mpj_exp_fdlibm(a); break;
    case 17: r = mpj_tan_bl(a); break;
    case 18: r = mpj_atan2_sel(a, y[i]); break;
    case 19: { double s, c; int b = 0; mpj_sincos_wide(a, &s, &c, &b); r = b ? mpj_sin(a) : s; break; }
    case 20: { double s, c; int b = 0; mpj_sincos_wide(a, &s, &c, &b); r = b ? mpj_cos(a) : c; break; }
    case 21: { int b = 0; r = mpj_tan_wide(a, &b); r = b ? mpj_tan(a) : r; break; }
    case 22: r = mpj_sin_34(a); break;
    case 23: r = mpj_log_bl(a); break;
    case 24: r = mpj_atan_rows(a, arows); break;
    // exact cheap divisions a / y[i] (must equal `/`): guarded; hoisted reciprocal with the divisor checked
    // by the caller; the same with the fixup taking zero, Inf and NaN numerators; the shared-reciprocal pair
    case 25: r = mpj_div_g(a, y[i]); break;
    case 26: r = mpj_div_gn(a, y[i], mpj_rcp_nr(y[i]), !mpj_div_out(y[i])); break;
    case 27: r = mpj_div_gf(a, y[i], mpj_rcp_nr(y[i]), !mpj_div_out(y[i])); break;
    case 28: { double q1, q2; mpj_div2_g(a, 1.0, y[i], &q1, &q2); r = q1; break; }
    case 29: { double q1, q2; mpj_div2_g(-1.5, a, y[i], &q1, &q2); r = q2; break; }
    // what v_div_scale_f64 does to a / y[i]: 1 numerator changed + 2 divisor changed + 4 VCC set (either call)
    case 30: {
      bool v0 = false, v1 = false;
      const double dn = __builtin_amdgcn_div_scale(a, y[i], true, &v0);
      const double dd = __builtin_amdgcn_div_scale(a, y[i], false, &v1);
      const unsigned long long ua = (unsigned long long)__double_as_longlong(a), ud = (unsigned long long)__double_as_longlong(y[i]);
      r = (double)(((unsigned long long)__double_as_longlong(dn) != ua ? 1 : 0) +
                   ((unsigned long long)__double_as_longlong(dd) != ud ? 2 : 0) + ((v0 || v1) ? 4 : 0));
      break;
    }
  }
  out[i] = r;
}
bool two_op(int fn) { return fn == 4 || fn == 18 || fn >= 25; }

// One thread per row-major 2x2.  mpj_pinv2_bl's exact fallback is wave-uniform (MPJ_ANY), so what a lane
// computes in mode 1 depends on the matrices of the other lanes of its wave; the lanes past n have left.
__global__ __launch_bounds__(256) void pinv2_kernel(int mode, long long n, const double* M, double* out, int* rare) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double m[4] = {M[4 * i], M[4 * i + 1], M[4 * i + 2], M[4 * i + 3]};
  if (mode == 3) {
    double U[4], S[2], VT[4];
    mpj_svd2(m, U, S, VT);
    double* o = out + 10 * i;
    for (int c = 0; c < 4; c++) { o[c] = U[c]; o[6 + c] = VT[c]; }
    o[4] = S[0];
    o[5] = S[1];
    return;
  }
  double P[4];
  int ra = 0;
  if (mode == 0) mpj_pinv2(m, P);
  else if (mode == 1) mpj_pinv2_bl(m, P);
  else mpj_pinv2_fast(m, P, &ra);
  for (int c = 0; c < 4; c++) out[4 * i + c] = P[c];
  if (rare) rare[i] = mode == 2 ? (ra != 0) : 0;
}
}  // namespace

extern "C" int mp_math_eval(mp_ctx* ctx, int32_t fn, int64_t n, const double* x, const double* y, double* out) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, fn >= 0 && fn <= 30 && n >= 0 && x && out && (!two_op(fn) || y), "bad mp_math_eval arguments");
  if (n == 0) return MP_OK;
  MP_HIP(ctx, hipSetDevice(ctx->device));
  int st = MP_OK;
  const double* dx = mp_upload(ctx, WS_IO0, x, (size_t)n, &st);
  const double* dy = mp_upload(ctx, WS_IO1, two_op(fn) ? y : nullptr, (size_t)n, &st);
  double* dout = mp_alloc_out(ctx, WS_IO2, out, (size_t)n, &st);
  if (st) return st;
  hipLaunchKernelGGL(math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, fn, (long long)n, dx,
                     dy, dout);
  MP_HIP(ctx, hipGetLastError());
  if ((st = mp_download(ctx, out, (const double*)dout, (size_t)n))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}

extern "C" int mp_pinv2_eval(mp_ctx* ctx, int32_t mode, int64_t n, const double* M, double* out, int32_t* rare) {
  if (!ctx) return MP_ERR_INVALID;
  MP_CHECK(ctx, mode >= 0 && mode <= 3 && n >= 0 && n <= (int64_t)1 << 24 && M && out, "bad mp_pinv2_eval arguments");
  if (n == 0) return MP_OK;
  MP_HIP(ctx, hipSetDevice(ctx->device));
  int st = MP_OK;
  const size_t per = mode == 3 ? 10 : 4;
  const double* dM = mp_upload(ctx, WS_IO0, M, 4 * (size_t)n, &st);
  double* dout = mp_alloc_out(ctx, WS_IO1, out, per * (size_t)n, &st);
  int* drare = mp_alloc_out(ctx, WS_IO2, (int*)rare, (size_t)n, &st);
  if (st) return st;
  hipLaunchKernelGGL(pinv2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)mode, (long long)n,
                     dM, dout, drare);
  MP_HIP(ctx, hipGetLastError());
  if ((st = mp_download(ctx, out, (const double*)dout, per * (size_t)n))) return st;
  if ((st = mp_download(ctx, (int*)rare, (const int*)drare, (size_t)n))) return st;
  MP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MP_OK;
}
