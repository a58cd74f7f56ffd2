// Trial rows conv (include/smpq.h, "trial rows conv"): the listed output channels of one conv, from
// its packed operand, written in place into limb planes the caller holds, and the restore. A trial
// of a block's last conv changes one channel of the next block's kept input (smpq/suffix.py); this
// computes that channel alone instead of running the block again.
//
// Grid (pixel tiles of 64) x rows, 256 threads: four lanes share a pixel, each lane reads one 16-B
// piece of every 64-B K step of every activation limb plane (K is contiguous per pixel for 1x1 and
// per tap for 3x3) and the matching 16 B of the row's weight limbs from LDS (staged once per block),
// and accumulates the kept (activation limb, weight limb) passes with v_dot4_i32_i8 into the conv's
// NACC int32 sums (conv_common.h limb_smin / limb_nacc). Integer sums are exact, so their order is
// free; two lane exchanges fold the four partial sums, and one lane per pixel runs the conv's own
// epilogue arithmetic (lds_dma.h lean_v1 / lean_zr / lean_clamp), saves the old digit bytes and stores the new
// ones. The kernel moves the conv's activation bytes once per row and one channel's results: no
// tuning table. Plain vector stores only.
#include <cstring>

#include "lds_dma.h"
#include "trial_row_host.h"

namespace smpq {
namespace {

constexpr int kTcThreads = 256;
constexpr int kTcPix = kTcThreads / 4;  // pixels per block

struct TrialConvArgs {
  const int8_t* xq;
  const float* x_absmax;
  const int8_t* codes;
  const float* col_scale;
  const float* col_shift;
  const int8_t* res_q;
  const int32_t* channels;
  int8_t* yq;
  int8_t* save;
  int32_t* overflow;
  long long plane, wplane, oplane;  // bytes per activation / weight / output limb plane
  int M, h, w, cin, cout, K;
  float res_scale, yq_inv, inv_qmax;
};

template <int L, int LW, bool K3>
__global__ __launch_bounds__(kTcThreads) void trial_rows_conv_kernel(TrialConvArgs a) {
  constexpr int SMIN = limb_smin(L, LW), NACC = limb_nacc(L, LW);
  extern __shared__ __attribute__((aligned(16))) int8_t wrow[];  // [LW][K]: the row's weight limbs
  const int row = blockIdx.y;
  const int c = a.channels[row];
  if (c < 0 || c >= a.cout) return;  // (block-uniform) a list entry out of range: nothing is touched
  const int K = a.K, k16 = K >> 4;
  for (int i = threadIdx.x; i < LW * k16; i += kTcThreads) {
    const int lw = i / k16, p = i - lw * k16;
    reinterpret_cast<int4*>(wrow)[i] =
        *reinterpret_cast<const int4*>(a.codes + lw * a.wplane + (long long)c * K + 16 * p);
  }
  __syncthreads();

  const int sub = threadIdx.x & 3;
  const long long m = (long long)blockIdx.x * kTcPix + (threadIdx.x >> 2);
  const bool ok = m < a.M;
  const int hw = a.h * a.w;
  const int g = ok ? (int)(m / hw) : 0;
  int acc[NACC];
#pragma unroll
  for (int t = 0; t < NACC; ++t) acc[t] = 0;
  if (ok) {
    const int rem = (int)(m - (long long)g * hw), oy = rem / a.w, ox = rem - oy * a.w;
    const int steps = a.cin >> 6;
#pragma unroll 1
    for (int tap = 0; tap < (K3 ? 9 : 1); ++tap) {
      long long src = m;
      if (K3) {
        const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        if (iy < 0 || iy >= a.h || ix < 0 || ix >= a.w) continue;  // a tap outside the image adds zero
        src = ((long long)g * a.h + iy) * a.w + ix;
      }
      const int8_t* xp = a.xq + src * a.cin + 16 * sub;
      const int8_t* wp = wrow + tap * a.cin + 16 * sub;
#pragma unroll 2
      for (int s = 0; s < steps; ++s) {
        v4i xv[L], wv[LW];
#pragma unroll
        for (int l = 0; l < L; ++l) xv[l] = *reinterpret_cast<const v4i*>(xp + l * a.plane + 64 * s);
#pragma unroll
        for (int lw = 0; lw < LW; ++lw) wv[lw] = *reinterpret_cast<const v4i*>(wp + lw * K + 64 * s);
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
          for (int lw = 0; lw < LW; ++lw) {
            if (l + lw < SMIN) continue;  // compile-time: the low-digit products the conv kernels skip
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[l + lw - SMIN] = __builtin_amdgcn_sdot4(xv[l][j], wv[lw][j], acc[l + lw - SMIN], false);
          }
      }
    }
  }
  // the four lanes of a pixel hold partial sums (all lanes take part; lanes past M hold zeros)
#pragma unroll
  for (int t = 0; t < NACC; ++t) {
    acc[t] += __shfl_xor(acc[t], 1, kWave);
    acc[t] += __shfl_xor(acc[t], 2, kWave);
  }
  bool ovf = false;
  if (ok && sub == 0) {
    constexpr float qmax = act_qmax<L>();
    const float inv = a.yq_inv;
    const float csq = a.col_scale[c] * inv, shq = a.col_shift[c] * inv, rsq = a.res_scale * inv;
    const float rscale = a.x_absmax[g] * a.inv_qmax;
    const long long at = m * a.cout + c;
    int rq = 0;
    if (a.res_q) {
#pragma unroll
      for (int l = L - 1; l >= 0; --l) rq = rq * 256 + (int)a.res_q[l * a.oplane + at];
    }
    v4i accs[NACC];
#pragma unroll
    for (int t = 0; t < NACC; ++t) accs[t] = v4i{acc[t], 0, 0, 0};
    const float zr = lean_zr(lean_v1<NACC, SMIN>(accs, 0), rscale, csq, shq, a.res_q != nullptr, &rq, 0, rsq);
    ovf = zr > qmax;
    const int q = lean_clamp<L>(zr, 0.f);
    int d[L];
    split_limbs<L>(q, d);
    int8_t* slot = a.save + (long long)row * L * a.M + m;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      slot[(long long)l * a.M] = a.yq[l * a.oplane + at];
      a.yq[l * a.oplane + at] = (int8_t)d[l];
    }
  }
  if (__any(ovf) && (threadIdx.x & (kWave - 1)) == 0) atomicMax(a.overflow, 1);
}

// one thread per saved byte: (row, limb, pixel)
__global__ __launch_bounds__(kTcThreads) void trial_rows_conv_restore_kernel(const int32_t* channels, int nrows,
                                                                             int limbs, long long pixels, int cout,
                                                                             int8_t* yq, const int8_t* save) {
  const long long i = (long long)blockIdx.x * kTcThreads + threadIdx.x;
  if (i >= (long long)nrows * limbs * pixels) return;
  const long long rl = i / pixels, m = i - rl * pixels;
  const int row = (int)(rl / limbs), l = (int)(rl - (long long)row * limbs);
  const int c = channels[row];
  if (c < 0 || c >= cout) return;
  yq[((long long)l * pixels + m) * cout + c] = save[i];
}

template <int L, int LW>
int launch_trial_conv(const TrialConvArgs& a, bool k3, int nrows, hipStream_t s) {
  const dim3 grid((unsigned)((a.M + kTcPix - 1) / kTcPix), (unsigned)nrows);
  const size_t lds = (size_t)LW * a.K;
  if (k3)
    hipLaunchKernelGGL((trial_rows_conv_kernel<L, LW, true>), grid, dim3(kTcThreads), lds, s, a);
  else
    hipLaunchKernelGGL((trial_rows_conv_kernel<L, LW, false>), grid, dim3(kTcThreads), lds, s, a);
  return check_hip(hipGetLastError(), "trial_rows_conv_kernel launch");
}

}  // namespace
}  // namespace smpq

using namespace smpq;

extern "C" int smpq_trial_rows_conv_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                      const int8_t* codes, int wlimbs, int cout, int kh, int kw, int stride, int pad,
                                      const float* col_scale, const float* col_shift, int limbs,
                                      const int8_t* residual_q, float residual_range, const int32_t* channels,
                                      int nrows, int8_t* yq, float yq_range, int32_t* overflow, void* save,
                                      smpq_stream_t stream) {
  std::string err;
  const int rc = trial_rows_conv_check("smpq_trial_rows_conv_q", xq, x_absmax, n, h, w, cin, codes, wlimbs, cout, kh,
                                       kw, stride, pad, col_scale, col_shift, limbs, residual_q, residual_range,
                                       channels, nrows, yq, yq_range, overflow, save, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  const float qmax = limbs == 2 ? 32512.f : 8323072.f;
  TrialConvArgs a{};
  a.xq = xq;
  a.x_absmax = x_absmax;
  a.codes = codes;
  a.col_scale = col_scale;
  a.col_shift = col_shift;
  a.res_q = residual_q;
  a.channels = channels;
  a.yq = yq;
  a.save = static_cast<int8_t*>(save);
  a.overflow = overflow;
  a.M = n * h * w;
  a.h = h;
  a.w = w;
  a.cin = cin;
  a.cout = cout;
  a.K = cin * kh * kw;
  a.plane = (long long)a.M * cin;
  a.wplane = (long long)cout * a.K;
  a.oplane = (long long)a.M * cout;
  // the conv's own host-side constants (conv.hip conv_args_q)
  a.res_scale = residual_q ? residual_range / qmax : 0.f;
  a.yq_inv = qmax / yq_range;
  a.inv_qmax = 1.f / qmax;
  const bool k3 = kh == 3;
  hipStream_t s = (hipStream_t)stream;
  if (limbs == 3 && wlimbs == 3) return launch_trial_conv<3, 3>(a, k3, nrows, s);
  if (limbs == 3) return launch_trial_conv<3, 2>(a, k3, nrows, s);
  return launch_trial_conv<2, 2>(a, k3, nrows, s);
}

extern "C" int smpq_trial_rows_conv_restore(const int32_t* channels, int nrows, int limbs, int64_t pixels, int cout,
                                            int8_t* yq, const void* save, smpq_stream_t stream) {
  std::string err;
  const int rc = trial_rows_conv_restore_check("smpq_trial_rows_conv_restore", channels, nrows, limbs, pixels, cout, yq,
                                               save, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  const long long total = (long long)nrows * limbs * pixels;
  hipLaunchKernelGGL(trial_rows_conv_restore_kernel, dim3((unsigned)((total + kTcThreads - 1) / kTcThreads)),
                     dim3(kTcThreads), 0, (hipStream_t)stream, channels, nrows, limbs, (long long)pixels, cout, yq,
                     static_cast<const int8_t*>(save));
  return check_hip(hipGetLastError(), "trial_rows_conv_restore_kernel launch");
}

extern "C" int smpq_trial_rows_conv_q_host(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                           const int8_t* codes, int wlimbs, int cout, int kh, int kw, int stride,
                                           int pad, const float* col_scale, const float* col_shift, int limbs,
                                           const int8_t* residual_q, float residual_range, const int32_t* channels,
                                           int nrows, int8_t* yq, float yq_range, int32_t* overflow, void* save) {
  std::string err;
  const int rc = trial_rows_conv_host(xq, x_absmax, n, h, w, cin, codes, wlimbs, cout, kh, kw, stride, pad, col_scale,
                                      col_shift, limbs, residual_q, residual_range, channels, nrows, yq, yq_range,
                                      overflow, save, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}

extern "C" int smpq_trial_rows_conv_restore_host(const int32_t* channels, int nrows, int limbs, int64_t pixels,
                                                 int cout, int8_t* yq, const void* save) {
  std::string err;
  const int rc = trial_rows_conv_restore_host(channels, nrows, limbs, pixels, cout, yq, save, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}
