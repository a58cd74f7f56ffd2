// Weight fake-quantizer (bit-exact with the reference) and the int8 code packer.
//
// Reference arithmetic (functions.py:25-43, quantize_wgt), per output channel t:
//   mn, mx  = exact fp32 min / max of t                      (functions.py:35-36, .item())
//   scale   = (mx - mn) / (2^bit - 1)           IEEE double   (functions.py:39)
//   z       = round(mn / scale)                 half-even      (functions.py:40)
//   q       = (rne(t / f32(scale) + f32(z)) - f32(z)) * f32(scale)   fp32 ops (functions.py:41)
// What `t / scale` (scale a Python float) rounds to depends on where the reference's tensor lives:
//   SMPQ_QSEM_CPU     torch CPU: a correctly rounded fp32 division t / f32(scale) (__fdiv_rn);
//   SMPQ_QSEM_DEVICE  torch on the GPU: t * f32(1.0 / scale), a multiply by the reciprocal of the
//                     DOUBLE scale rounded once to fp32 (ATen's tensor-by-scalar division on
//                     device; pinned by tests/golden/quant_kat_device.npz, which torch itself
//                     produced on an MI355X: 2 of the 69 KAT channels round differently there).
// The reference's drivers quantize channels of a model already moved to the GPU
// (functions.py:97 net.to(device) before resnet50_main.py:189-197), so device tensors default to
// SMPQ_QSEM_DEVICE and host tensors to SMPQ_QSEM_CPU (smpq.quant). FP contraction is off.
//
// One workgroup per output channel: channels are at most 4608 elements (R50 layer4 conv2),
// so a 256-thread block covers a channel in <= 18 iterations and the launch is a single
// wave of blocks over all channels of a layer (22,656 channels for all of ResNet-50).
#include <cmath>
#include <cstring>
#include <string>

#include "common.h"
#include "trial_row_host.h"

#pragma clang fp contract(off)

namespace smpq {

constexpr int kQThreads = 256;

__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* smem) {
  // smem: 2 * (kQThreads / 64) floats
  mn = wave_min(mn);
  mx = wave_max(mx);
  const int wid = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    smem[wid] = mn;
    smem[kQThreads / kWave + wid] = mx;
  }
  __syncthreads();
  mn = smem[0];
  mx = smem[kQThreads / kWave];
#pragma unroll
  for (int i = 1; i < kQThreads / kWave; ++i) {
    mn = fminf(mn, smem[i]);
    mx = fmaxf(mx, smem[kQThreads / kWave + i]);
  }
}

__global__ __launch_bounds__(kQThreads) void quantize_channels_kernel(
    float* __restrict__ w, int k, const int8_t* __restrict__ bits, float* __restrict__ scale_out,
    int32_t* __restrict__ status, int semantics) {
  __shared__ float smem[2 * kQThreads / kWave];
  const int c = blockIdx.x;
  const int b = bits[c];
  if (b <= 0) return;
  float* row = w + (size_t)c * k;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < k; i += kQThreads) {
    const float v = row[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, smem);
  if (mx == mn) {  // reference: ZeroDivisionError at functions.py:40
    // status keeps the LOWEST constant channel + 1, whatever order the blocks arrive in: store
    // c + 1 over 0 or over a higher channel's report, give way to a lower one
    if (threadIdx.x == 0) {
      int* st = reinterpret_cast<int*>(status);
      int seen = 0;
      for (;;) {
        const int old = atomicCAS(st, seen, c + 1);
        if (old == seen || (old != 0 && old <= c + 1)) break;
        seen = old;
      }
    }
    return;
  }
  const double scale = ((double)mx - (double)mn) / (double)((1 << b) - 1);
  const double zd = rint((double)mn / scale) + 0.0;  // Python round(): half-to-even; no -0
  const float s32 = (float)scale;
  const float z32 = (float)zd;
  const float inv32 = (float)(1.0 / scale);
  const bool dev = semantics == SMPQ_QSEM_DEVICE;
  for (int i = threadIdx.x; i < k; i += kQThreads) {
    const float t = row[i];
    const float d = dev ? __fmul_rn(t, inv32) : __fdiv_rn(t, s32);
    const float q = rintf(d + z32) - z32;
    row[i] = __fmul_rn(q, s32);
  }
  if (threadIdx.x == 0) scale_out[c] = s32;
}

// Weight codes for the conv's B operand, one workgroup per output channel.
//   w [cout][cin][kh][kw] fp32, step [cout] (0 = channel never quantized).
//   Exact mode (step > 0 and every w == fl32(m * step), |m| <= WMAX): the integer codes m of
//     the reference quantizer (functions.py:41) — recovered by m = rne(w / step), exact because
//     |w / step - m| < 2^-14 — verified bitwise.
//   Fixed mode (lw >= 2: unquantized / off-grid channels): per-channel fixed point with
//     WMAX = 32512 (lw 2, 16-bit) or 8323072 (lw 3, 24-bit): wscale = max|w| / WMAX,
//     m = rne(w / wscale).
//   lw == 1: m - offset stored as one int8 plane (offset != 0 only when [min m, max m] is not
//     inside [-128, 127]); lw >= 2: m stored as lw balanced int8 digit planes, no offset.
//   lw >= 2, exact channels: m is shifted left by the most bits that keep max|m| << sh <= WMAX
//     (wscale = step * 2^-sh, exact), so every channel's magnitude sits in the TOP weight limb.
//     The conv kernels skip the low-digit products (limb pairs l + lw < L + LW - 4); without the
//     shift an 8-bit code would live in limb 0 alone and lose the low activation limbs entirely
//     (a mixed exact / fixed-point conv of a mid-search layer was off by ~1e-3 of its logits).
//     The shift changes no value (m * step == (m << sh) * (step * 2^-sh) exactly), only which
//     limb products carry it.
//   Layout: codes[l][c][k], k = tap * cin_pad + ci (tap = r * kw + q), zero-padded to K.
//   status[0] += off-grid channels (lw == 1: error), status[1] += channels whose exact codes do
//   not fit (lw == 1: > 256 levels), status[2] += channels coded in fixed mode.
constexpr float kW16Max = 32512.f;    // 2-limb fixed-point code range (127 * 256)
constexpr float kW24Max = 8323072.f;  // 3-limb fixed-point code range (127 * 65536)

__global__ __launch_bounds__(kQThreads) void pack_weights_ex_kernel(
    const float* __restrict__ w, int cin, int kh, int kw, int cin_pad, int K, int lw, int s2d,
    const float* __restrict__ step, int8_t* __restrict__ codes, long long wplane,
    int32_t* __restrict__ offset, float* __restrict__ wscale, int32_t* __restrict__ status) {
  __shared__ int smem[4 * kQThreads / kWave];
  __shared__ float sabs[kQThreads / kWave];
  const int c = blockIdx.x;
  const int taps = kh * kw;
  const int kreal = cin * taps;
  const float* row = w + (size_t)c * kreal;
  const float s = step ? step[c] : 0.f;
  const float wmax = lw >= 3 ? kW24Max : kW16Max;
  int mmin = INT32_MAX, mmax = INT32_MIN, bad = (s > 0.f) ? 0 : 1;
  float amax = 0.f;
  for (int i = threadIdx.x; i < kreal; i += kQThreads) {
    const float v = row[i];
    amax = fmaxf(amax, fabsf(v));
    if (bad) continue;
    const float mf = rintf(__fdiv_rn(v, s));
    if (__fmul_rn(mf, s) != v || fabsf(mf) > wmax) {
      bad = 1;
      continue;
    }
    mmin = min(mmin, (int)mf);
    mmax = max(mmax, (int)mf);
  }
  mmin = wave_min_i(mmin);
  mmax = wave_max_i(mmax);
  bad = wave_max_i(bad);
  amax = wave_max(amax);
  const int wid = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    smem[wid] = mmin;
    smem[4 + wid] = mmax;
    smem[8 + wid] = bad;
    sabs[wid] = amax;
  }
  __syncthreads();
  mmin = min(min(smem[0], smem[1]), min(smem[2], smem[3]));
  mmax = max(max(smem[4], smem[5]), max(smem[6], smem[7]));
  bad = smem[8] | smem[9] | smem[10] | smem[11];
  amax = fmaxf(fmaxf(sabs[0], sabs[1]), fmaxf(sabs[2], sabs[3]));
  int o = 0;
  bool fixed = false, range_bad = false;
  float sc = s;
  if (lw == 1) {
    if (!bad) {
      if (mmax - mmin > 255) range_bad = true;
      else if (mmin < -128 || mmax > 127) o = mmin + 128;
    }
  } else if (bad) {
    fixed = true;
    sc = amax > 0.f ? amax / wmax : 1.f;
  }
  int sh = 0;  // lw >= 2, exact channel: normalize the codes into the top limb
  if (lw >= 2 && !bad) {
    const int am = max(abs(mmin), abs(mmax));
    const int lim = (int)wmax;
    while (am > 0 && sh < 8 * (lw - 1) && (am << (sh + 1)) <= lim) ++sh;
    sc = ldexpf(s, -sh);
  }
  if (threadIdx.x == 0) {
    if (bad && s > 0.f) atomicAdd(&status[0], 1);
    if (lw == 1 && bad && !(s > 0.f)) atomicAdd(&status[0], 1);
    if (range_bad) atomicAdd(&status[1], 1);
    if (fixed) atomicAdd(&status[2], 1);
    if (offset) offset[c] = o;
    if (wscale) wscale[c] = sc;
  }
  const bool zero = (lw == 1) && (bad || range_bad);
  for (int k = threadIdx.x; k < K; k += kQThreads) {
    int src = -1;  // index of the weight in the [cin][kh][kw] row, or -1 for a zero code
    if (s2d) {
      // space-to-depth stem (smpq_pack_weights_s2d): k = [ty][tx][dy][dx][c] over a 4 x 4 x 16
      // kernel; original tap (2 ty + dy - 1, 2 tx + dx - 1) of channel c
      const int t = k >> 4, ch = k & 15;
      const int kr = 2 * (t >> 2) + (ch >> 3) - 1, kc = 2 * (t & 3) + ((ch >> 2) & 1) - 1, ci = ch & 3;
      if (ci < cin && kr >= 0 && kr < kh && kc >= 0 && kc < kw) src = ci * taps + kr * kw + kc;
    } else {
      const int tap = k / cin_pad;
      const int ci = k - tap * cin_pad;
      if (tap < taps && ci < cin) src = ci * taps + tap;
    }
    int m = 0;
    if (!zero && src >= 0) {
      const float v = row[src];
      // fixed point: round in double (at 24 bits an fp32 quotient cannot round exactly)
      if (fixed) m = (int)fmin(fmax(rint((double)v / (double)sc), -(double)wmax), (double)wmax);
      else m = ((int)rintf(__fdiv_rn(v, s)) - o) * (1 << sh);
    }
    for (int l = 0; l < lw; ++l) {  // balanced base-256 digits (the last one takes the rest)
      const int lo = (l == lw - 1) ? m : ((m + 128) & 255) - 128;
      codes[l * wplane + (size_t)c * K + k] = (int8_t)lo;
      m = (m - lo) >> 8;
    }
  }
}

// Trial row patch (include/smpq.h): channel c of a packed operand (lw >= 2) overwritten with what
// quantize_channels_kernel at `b` bits followed by pack_weights_ex_kernel with that step would
// have packed, the fp32 weight only read. The two kernels' arithmetic is restated here (the
// quantized row lives in LDS instead of the weight), not shared, so their code is untouched.
// One workgroup per row. A thread saves and rewrites the same (l, k) bytes and thread 0 the two
// scalars, so no store is ordered against another thread's load; rows of distinct channels share
// no byte, so nothing is ordered across workgroups either. The body exists once, for the single-row
// kernel and the n-row one.
__device__ __forceinline__ void trial_row_patch_body(
    const float* __restrict__ w, int cout, int cin, int taps, int c, int b, int semantics, int lw,
    const float* __restrict__ bn_a, int8_t* __restrict__ codes, int8_t* __restrict__ km,
    float* __restrict__ wscale, float* __restrict__ col_scale, float* __restrict__ save_head,
    int8_t* __restrict__ save_codes, int32_t* __restrict__ status) {
  __shared__ float qrow[SMPQ_TRIAL_MAX_K];
  __shared__ float smem[2 * kQThreads / kWave];
  __shared__ int ismem[3 * kQThreads / kWave];
  __shared__ float sabs[kQThreads / kWave];
  const int K = cin * taps;
  const size_t wplane = (size_t)cout * K;
  const float* row = w + (size_t)c * K;
  for (int k = threadIdx.x; k < K; k += kQThreads)
    for (int l = 0; l < lw; ++l) save_codes[(size_t)l * K + k] = codes[l * wplane + (size_t)c * K + k];
  if (threadIdx.x == 0) {
    save_head[0] = wscale[c];
    save_head[1] = col_scale[c];
  }
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < K; i += kQThreads) {
    const float v = row[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, smem);
  if (mx == mn) {  // constant channel: reported, the operand left as it is
    if (threadIdx.x == 0) status[0] = 1;
    return;
  }
  // quantize_channels_kernel
  const double scale = ((double)mx - (double)mn) / (double)((1 << b) - 1);
  const double zd = rint((double)mn / scale) + 0.0;
  const float s = (float)scale;
  const float z32 = (float)zd;
  const float inv32 = (float)(1.0 / scale);
  const bool dev = semantics == SMPQ_QSEM_DEVICE;
  const float wmax = lw >= 3 ? kW24Max : kW16Max;
  // ... and pack_weights_ex_kernel's on-grid check of the same element, step s
  int mmin = INT32_MAX, mmax = INT32_MIN, bad = (s > 0.f) ? 0 : 1;
  float amax = 0.f;
  for (int i = threadIdx.x; i < K; i += kQThreads) {
    const float t = row[i];
    const float d = dev ? __fmul_rn(t, inv32) : __fdiv_rn(t, s);
    const float q = rintf(d + z32) - z32;
    const float v = __fmul_rn(q, s);
    qrow[i] = v;
    amax = fmaxf(amax, fabsf(v));
    if (bad) continue;
    const float mf = rintf(__fdiv_rn(v, s));
    if (__fmul_rn(mf, s) != v || fabsf(mf) > wmax) {
      bad = 1;
      continue;
    }
    mmin = min(mmin, (int)mf);
    mmax = max(mmax, (int)mf);
  }
  mmin = wave_min_i(mmin);
  mmax = wave_max_i(mmax);
  bad = wave_max_i(bad);
  amax = wave_max(amax);
  const int wid = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    ismem[wid] = mmin;
    ismem[4 + wid] = mmax;
    ismem[8 + wid] = bad;
    sabs[wid] = amax;
  }
  __syncthreads();  // (also: qrow is complete)
  mmin = min(min(ismem[0], ismem[1]), min(ismem[2], ismem[3]));
  mmax = max(max(ismem[4], ismem[5]), max(ismem[6], ismem[7]));
  bad = ismem[8] | ismem[9] | ismem[10] | ismem[11];
  amax = fmaxf(fmaxf(sabs[0], sabs[1]), fmaxf(sabs[2], sabs[3]));
  const bool fixed = bad != 0;
  float sc = s;
  int sh = 0;
  if (fixed) {
    sc = amax > 0.f ? amax / wmax : 1.f;
  } else {
    const int am = max(abs(mmin), abs(mmax));
    const int lim = (int)wmax;
    while (am > 0 && sh < 8 * (lw - 1) && (am << (sh + 1)) <= lim) ++sh;
    sc = ldexpf(s, -sh);
  }
  const int kc = K / 64;
  for (int k = threadIdx.x; k < K; k += kQThreads) {
    const int tap = k / cin;
    const int ci = k - tap * cin;
    const float v = qrow[ci * taps + tap];
    int m;
    if (fixed) m = (int)fmin(fmax(rint((double)v / (double)sc), -(double)wmax), (double)wmax);
    else m = (int)rintf(__fdiv_rn(v, s)) * (1 << sh);
    for (int l = 0; l < lw; ++l) {
      const int lo = (l == lw - 1) ? m : ((m + 128) & 255) - 128;
      codes[l * wplane + (size_t)c * K + k] = (int8_t)lo;
      if (km) km[(((size_t)l * kc + (k >> 6)) * cout + c) * 64 + (k & 63)] = (int8_t)lo;
      m = (m - lo) >> 8;
    }
  }
  if (threadIdx.x == 0) {
    wscale[c] = sc;
    col_scale[c] = __fmul_rn(sc, bn_a[c]);
  }
}

__global__ __launch_bounds__(kQThreads) void trial_row_patch_kernel(
    const float* __restrict__ w, int cout, int cin, int taps, int c, int b, int semantics, int lw,
    const float* __restrict__ bn_a, int8_t* __restrict__ codes, int8_t* __restrict__ km,
    float* __restrict__ wscale, float* __restrict__ col_scale, float* __restrict__ save_head,
    int8_t* __restrict__ save_codes, int32_t* __restrict__ status) {
  trial_row_patch_body(w, cout, cin, taps, c, b, semantics, lw, bn_a, codes, km, wscale, col_scale, save_head,
                       save_codes, status);
}

// Workgroup i: row channels[i] at bits[i] bits, save slot i (``slot`` bytes each), status[i]. The
// lists are the caller's (distinct channels in [0, cout), bits in 1..16); an entry outside those
// ranges touches nothing and reports 2, so a bad list cannot write out of bounds.
__global__ __launch_bounds__(kQThreads) void trial_rows_patch_kernel(
    const float* __restrict__ w, int cout, int cin, int taps, const int32_t* __restrict__ channels,
    const int32_t* __restrict__ bits, int semantics, int lw, const float* __restrict__ bn_a,
    int8_t* __restrict__ codes, int8_t* __restrict__ km, float* __restrict__ wscale, float* __restrict__ col_scale,
    int8_t* __restrict__ save, long long slot, int32_t* __restrict__ status) {
  const int i = blockIdx.x;
  const int c = channels[i], b = bits[i];
  if (c < 0 || c >= cout || b < 1 || b > 16) {
    if (threadIdx.x == 0) status[i] = 2;
    return;
  }
  int8_t* s = save + (size_t)i * slot;
  trial_row_patch_body(w, cout, cin, taps, c, b, semantics, lw, bn_a, codes, km, wscale, col_scale,
                       reinterpret_cast<float*>(s), s + SMPQ_TRIAL_SAVE_HEADER, status + i);
}

__device__ __forceinline__ void trial_row_restore_body(
    int cout, int K, int c, int lw, int8_t* __restrict__ codes, int8_t* __restrict__ km,
    float* __restrict__ wscale, float* __restrict__ col_scale, const float* __restrict__ save_head,
    const int8_t* __restrict__ save_codes) {
  const size_t wplane = (size_t)cout * K;
  const int kc = K / 64;
  for (int k = threadIdx.x; k < K; k += kQThreads)
    for (int l = 0; l < lw; ++l) {
      const int8_t v = save_codes[(size_t)l * K + k];
      codes[l * wplane + (size_t)c * K + k] = v;
      if (km) km[(((size_t)l * kc + (k >> 6)) * cout + c) * 64 + (k & 63)] = v;
    }
  if (threadIdx.x == 0) {
    wscale[c] = save_head[0];
    col_scale[c] = save_head[1];
  }
}

__global__ __launch_bounds__(kQThreads) void trial_row_restore_kernel(
    int cout, int K, int c, int lw, int8_t* __restrict__ codes, int8_t* __restrict__ km,
    float* __restrict__ wscale, float* __restrict__ col_scale, const float* __restrict__ save_head,
    const int8_t* __restrict__ save_codes) {
  trial_row_restore_body(cout, K, c, lw, codes, km, wscale, col_scale, save_head, save_codes);
}

__global__ __launch_bounds__(kQThreads) void trial_rows_restore_kernel(
    int cout, int K, const int32_t* __restrict__ channels, int lw, int8_t* __restrict__ codes,
    int8_t* __restrict__ km, float* __restrict__ wscale, float* __restrict__ col_scale,
    const int8_t* __restrict__ save, long long slot) {
  const int c = channels[blockIdx.x];
  if (c < 0 || c >= cout) return;
  const int8_t* s = save + (size_t)blockIdx.x * slot;
  trial_row_restore_body(cout, K, c, lw, codes, km, wscale, col_scale, reinterpret_cast<const float*>(s),
                         s + SMPQ_TRIAL_SAVE_HEADER);
}

// Trial rows patch for an 'exact8' operand (include/smpq.h): one int8 plane, a per-channel offset
// read by the conv kernels at run time, wscale = the step. quantize_channels_kernel and the lw == 1
// branch of pack_weights_ex_kernel restated with step s, as above. Workgroup i: row channels[i] at
// bits[i] bits (1..8), slot i, status[i]; a row that the normal path would not pack exact8 (3) or
// that needs an offset the operand does not have (4) is reported and left as it is. A thread
// saves and rewrites the same k bytes and thread 0 the three scalars.
__global__ __launch_bounds__(kQThreads) void trial_rows_patch_x8_kernel(
    const float* __restrict__ w, int cout, int cin, int taps, const int32_t* __restrict__ channels,
    const int32_t* __restrict__ bits, int semantics, const float* __restrict__ bn_a, int8_t* __restrict__ codes,
    int8_t* __restrict__ km, int32_t* __restrict__ offset, float* __restrict__ wscale, float* __restrict__ col_scale,
    int8_t* __restrict__ save, long long slot, int32_t* __restrict__ status) {
  __shared__ float qrow[SMPQ_TRIAL_MAX_K];
  __shared__ float smem[2 * kQThreads / kWave];
  __shared__ int ismem[3 * kQThreads / kWave];
  const int i = blockIdx.x;
  const int c = channels[i], b = bits[i];
  if (c < 0 || c >= cout) {  // nothing of this entry can be addressed
    if (threadIdx.x == 0) status[i] = 2;
    return;
  }
  const int K = cin * taps;
  const float* row = w + (size_t)c * K;
  int8_t* crow = codes + (size_t)c * K;
  int8_t* sv = save + (size_t)i * slot;
  for (int k = threadIdx.x; k < K; k += kQThreads) sv[SMPQ_TRIAL_SAVE_HEADER + k] = crow[k];
  if (threadIdx.x == 0) {
    reinterpret_cast<float*>(sv)[0] = wscale[c];
    reinterpret_cast<float*>(sv)[1] = col_scale[c];
    reinterpret_cast<int32_t*>(sv)[2] = offset ? offset[c] : 0;
  }
  if (b < 1 || b > 8) {  // a wider row cannot be exact8
    if (threadIdx.x == 0) status[i] = 2;
    return;
  }
  float mn = INFINITY, mx = -INFINITY;
  for (int k = threadIdx.x; k < K; k += kQThreads) {
    const float v = row[k];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, smem);
  if (mx == mn) {  // constant channel
    if (threadIdx.x == 0) status[i] = 1;
    return;
  }
  const double scale = ((double)mx - (double)mn) / (double)((1 << b) - 1);
  const double zd = rint((double)mn / scale) + 0.0;
  const float s = (float)scale;
  const float z32 = (float)zd;
  const float inv32 = (float)(1.0 / scale);
  const bool dev = semantics == SMPQ_QSEM_DEVICE;
  int mmin = INT32_MAX, mmax = INT32_MIN, bad = (s > 0.f) ? 0 : 1;
  for (int k = threadIdx.x; k < K; k += kQThreads) {
    const float t = row[k];
    const float d = dev ? __fmul_rn(t, inv32) : __fdiv_rn(t, s);
    const float q = rintf(d + z32) - z32;
    const float v = __fmul_rn(q, s);
    qrow[k] = v;
    if (bad) continue;
    const float mf = rintf(__fdiv_rn(v, s));
    if (__fmul_rn(mf, s) != v || fabsf(mf) > kW16Max) {
      bad = 1;
      continue;
    }
    mmin = min(mmin, (int)mf);
    mmax = max(mmax, (int)mf);
  }
  mmin = wave_min_i(mmin);
  mmax = wave_max_i(mmax);
  bad = wave_max_i(bad);
  const int wid = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    ismem[wid] = mmin;
    ismem[4 + wid] = mmax;
    ismem[8 + wid] = bad;
  }
  __syncthreads();  // (also: qrow is complete)
  mmin = min(min(ismem[0], ismem[1]), min(ismem[2], ismem[3]));
  mmax = max(max(ismem[4], ismem[5]), max(ismem[6], ismem[7]));
  bad = ismem[8] | ismem[9] | ismem[10] | ismem[11];
  if (bad || mmax - mmin > 255) {  // the normal path would not pack this conv exact8
    if (threadIdx.x == 0) status[i] = 3;
    return;
  }
  const int o = (mmin < -128 || mmax > 127) ? mmin + 128 : 0;
  if (o != 0 && !offset) {
    if (threadIdx.x == 0) status[i] = 4;
    return;
  }
  for (int k = threadIdx.x; k < K; k += kQThreads) {
    const int tap = k / cin;
    const int ci = k - tap * cin;
    const int8_t code = (int8_t)((int)rintf(__fdiv_rn(qrow[ci * taps + tap], s)) - o);
    crow[k] = code;
    if (km) km[((size_t)(k >> 6) * cout + c) * 64 + (k & 63)] = code;
  }
  if (threadIdx.x == 0) {
    if (offset) offset[c] = o;
    wscale[c] = s;
    col_scale[c] = __fmul_rn(s, bn_a[c]);
  }
}

__global__ __launch_bounds__(kQThreads) void trial_rows_restore_x8_kernel(
    int cout, int K, const int32_t* __restrict__ channels, int8_t* __restrict__ codes, int8_t* __restrict__ km,
    int32_t* __restrict__ offset, float* __restrict__ wscale, float* __restrict__ col_scale,
    const int8_t* __restrict__ save, long long slot) {
  const int c = channels[blockIdx.x];
  if (c < 0 || c >= cout) return;
  const int8_t* sv = save + (size_t)blockIdx.x * slot;
  for (int k = threadIdx.x; k < K; k += kQThreads) {
    const int8_t v = sv[SMPQ_TRIAL_SAVE_HEADER + k];
    codes[(size_t)c * K + k] = v;
    if (km) km[((size_t)(k >> 6) * cout + c) * 64 + (k & 63)] = v;
  }
  if (threadIdx.x == 0) {
    wscale[c] = reinterpret_cast<const float*>(sv)[0];
    col_scale[c] = reinterpret_cast<const float*>(sv)[1];
    if (offset) offset[c] = reinterpret_cast<const int32_t*>(sv)[2];
  }
}

// ------------------------------------------------------------------------------------------
// host twin (native C++, same arithmetic)
// ------------------------------------------------------------------------------------------
static int quantize_row_host(float* row, int k, int b, float* s_out, int semantics) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < k; ++i) {
    mn = std::fmin(mn, row[i]);
    mx = std::fmax(mx, row[i]);
  }
  if (mx == mn) return SMPQ_E_CONSTANT;
  const double scale = ((double)mx - (double)mn) / (double)((1 << b) - 1);
  const double zd = std::nearbyint((double)mn / scale) + 0.0;
  const float s32 = (float)scale;
  const float z32 = (float)zd;
  const float inv32 = (float)(1.0 / scale);
  for (int i = 0; i < k; ++i) {
    // fp32 IEEE division, or the device's reciprocal multiply (contraction is off in this file)
    const float d = semantics == SMPQ_QSEM_DEVICE ? row[i] * inv32 : row[i] / s32;
    const float q = std::nearbyintf(d + z32) - z32;
    row[i] = q * s32;
  }
  *s_out = s32;
  return SMPQ_OK;
}

}  // namespace smpq

using namespace smpq;

extern "C" int smpq_quantize_channels_ex(float* w, int cout, int k_elems, const int8_t* bits,
                                         float* scale_out, int32_t* status, int semantics,
                                         smpq_stream_t stream) {
  if (!w || !bits || !scale_out || !status || cout <= 0 || k_elems <= 0)
    return fail(SMPQ_E_INVALID, "smpq_quantize_channels: bad arguments");
  if (semantics != SMPQ_QSEM_CPU && semantics != SMPQ_QSEM_DEVICE)
    return fail(SMPQ_E_INVALID, "smpq_quantize_channels: semantics must be SMPQ_QSEM_CPU or SMPQ_QSEM_DEVICE");
  hipLaunchKernelGGL(quantize_channels_kernel, dim3(cout), dim3(kQThreads), 0,
                     (hipStream_t)stream, w, k_elems, bits, scale_out, status, semantics);
  return check_hip(hipGetLastError(), "quantize_channels_kernel launch");
}

extern "C" int smpq_quantize_channels(float* w, int cout, int k_elems, const int8_t* bits,
                                      float* scale_out, int32_t* status, smpq_stream_t stream) {
  return smpq_quantize_channels_ex(w, cout, k_elems, bits, scale_out, status, SMPQ_QSEM_CPU, stream);
}

extern "C" int smpq_quantize_channels_host_ex(float* w, int cout, int k_elems, const int8_t* bits,
                                              float* scale_out, int semantics) {
  if (!w || !bits || cout <= 0 || k_elems <= 0)
    return fail(SMPQ_E_INVALID, "smpq_quantize_channels_host: bad arguments");
  if (semantics != SMPQ_QSEM_CPU && semantics != SMPQ_QSEM_DEVICE)
    return fail(SMPQ_E_INVALID, "smpq_quantize_channels_host: semantics must be SMPQ_QSEM_CPU or SMPQ_QSEM_DEVICE");
  for (int c = 0; c < cout; ++c) {
    const int b = bits[c];
    if (b <= 0) continue;
    if (b > 30) return fail(SMPQ_E_BITS, "smpq_quantize_channels_host: bit > 30");
    float* row = w + (size_t)c * k_elems;
    float s32 = 0.f;
    const int rc = quantize_row_host(row, k_elems, b, &s32, semantics);
    if (rc != SMPQ_OK)
      return fail(rc, "float division by zero (constant channel " + std::to_string(c) + ")");
    if (scale_out) scale_out[c] = s32;
  }
  return SMPQ_OK;
}

extern "C" int smpq_quantize_channels_host(float* w, int cout, int k_elems, const int8_t* bits,
                                           float* scale_out) {
  return smpq_quantize_channels_host_ex(w, cout, k_elems, bits, scale_out, SMPQ_QSEM_CPU);
}

extern "C" int smpq_pack_weights(const float* w, int cout, int cin, int kh, int kw,
                                 const float* step, int8_t* codes, int32_t* offset,
                                 int32_t* status, smpq_stream_t stream) {
  if (!w || !step || !codes || !offset || !status || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0)
    return fail(SMPQ_E_INVALID, "smpq_pack_weights: bad arguments");
  const int K = cin * kh * kw;
  hipLaunchKernelGGL(pack_weights_ex_kernel, dim3(cout), dim3(kQThreads), 0, (hipStream_t)stream, w,
                     cin, kh, kw, cin, K, 1, 0, step, codes, (long long)cout * K, offset, (float*)nullptr,
                     status);
  return check_hip(hipGetLastError(), "pack_weights_ex_kernel launch");
}

extern "C" int smpq_pack_weights_ex(const float* w, int cout, int cin, int kh, int kw, const float* step,
                                    int wlimbs, int8_t* codes, int32_t* offset, float* wscale,
                                    int32_t* status, smpq_stream_t stream) {
  if (!w || !codes || !wscale || !status || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0)
    return fail(SMPQ_E_INVALID, "smpq_pack_weights_ex: bad arguments");
  if (wlimbs < 1 || wlimbs > 3) return fail(SMPQ_E_INVALID, "smpq_pack_weights_ex: wlimbs must be 1, 2 or 3");
  if (wlimbs == 1 && (!step || !offset))
    return fail(SMPQ_E_INVALID, "smpq_pack_weights_ex: wlimbs == 1 needs step and offset");
  if (cin % 64 != 0)
    return fail(SMPQ_E_SHAPE,
                "smpq_pack_weights_ex: cin must be a multiple of 64 (the <= 4-channel stem: smpq_pack_weights_s2d_ex)");
  const int K = cin * kh * kw;
  hipLaunchKernelGGL(pack_weights_ex_kernel, dim3(cout), dim3(kQThreads), 0, (hipStream_t)stream, w,
                     cin, kh, kw, cin, K, wlimbs, 0, step, codes, (long long)cout * K, offset, wscale,
                     status);
  return check_hip(hipGetLastError(), "pack_weights_ex_kernel launch");
}

extern "C" int smpq_pack_weights_s2d_ex(const float* w, int cout, int cin, const float* step, int wlimbs,
                                        int8_t* codes, float* wscale, int32_t* status, smpq_stream_t stream) {
  if (!w || !codes || !wscale || !status || cout <= 0 || cin <= 0 || cin > 4)
    return fail(SMPQ_E_INVALID, "smpq_pack_weights_s2d: bad arguments (cin must be 1..4)");
  if (wlimbs < 2 || wlimbs > 3) return fail(SMPQ_E_INVALID, "smpq_pack_weights_s2d: wlimbs must be 2 or 3");
  constexpr int K = 256;  // 4 x 4 taps x 16 space-to-depth channels
  hipLaunchKernelGGL(pack_weights_ex_kernel, dim3(cout), dim3(kQThreads), 0, (hipStream_t)stream, w, cin, 7, 7,
                     16, K, wlimbs, 1, step, codes, (long long)cout * K, (int32_t*)nullptr, wscale, status);
  return check_hip(hipGetLastError(), "pack_weights_ex_kernel launch");
}

extern "C" int smpq_pack_weights_s2d(const float* w, int cout, int cin, int wlimbs, int8_t* codes, float* wscale,
                                     int32_t* status, smpq_stream_t stream) {
  return smpq_pack_weights_s2d_ex(w, cout, cin, nullptr, wlimbs, codes, wscale, status, stream);
}

extern "C" int smpq_trial_row_patch(const float* w, int cout, int cin, int kh, int kw, int channel, int bits,
                                    int semantics, int wlimbs, const float* bn_a, int8_t* codes, int8_t* codes_km,
                                    float* wscale, float* col_scale, void* save, int32_t* status,
                                    smpq_stream_t stream) {
  std::string err;
  const int rc = trial_row_check(w, cout, cin, kh, kw, channel, bits, semantics, wlimbs, bn_a, codes, wscale,
                                 col_scale, save, status, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  hipLaunchKernelGGL(trial_row_patch_kernel, dim3(1), dim3(kQThreads), 0, (hipStream_t)stream, w, cout, cin, kh * kw,
                     channel, bits, semantics, wlimbs, bn_a, codes, codes_km, wscale, col_scale,
                     static_cast<float*>(save), static_cast<int8_t*>(save) + SMPQ_TRIAL_SAVE_HEADER, status);
  return check_hip(hipGetLastError(), "trial_row_patch_kernel launch");
}

extern "C" int smpq_trial_row_restore(int cout, int K, int channel, int wlimbs, int8_t* codes, int8_t* codes_km,
                                      float* wscale, float* col_scale, const void* save, smpq_stream_t stream) {
  std::string err;
  const int rc = trial_restore_check(cout, K, channel, wlimbs, codes, wscale, col_scale, save, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  hipLaunchKernelGGL(trial_row_restore_kernel, dim3(1), dim3(kQThreads), 0, (hipStream_t)stream, cout, K, channel,
                     wlimbs, codes, codes_km, wscale, col_scale, static_cast<const float*>(save),
                     static_cast<const int8_t*>(save) + SMPQ_TRIAL_SAVE_HEADER);
  return check_hip(hipGetLastError(), "trial_row_restore_kernel launch");
}

extern "C" int smpq_trial_row_patch_host(const float* w, int cout, int cin, int kh, int kw, int channel, int bits,
                                         int semantics, int wlimbs, const float* bn_a, int8_t* codes, float* wscale,
                                         float* col_scale, void* save, int32_t* status) {
  std::string err;
  const int rc = trial_row_patch_host(w, cout, cin, kh, kw, channel, bits, semantics, wlimbs, bn_a, codes, wscale,
                                      col_scale, save, status, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}

extern "C" int smpq_trial_row_restore_host(int cout, int K, int channel, int wlimbs, int8_t* codes, float* wscale,
                                           float* col_scale, const void* save) {
  std::string err;
  const int rc = trial_row_restore_host(cout, K, channel, wlimbs, codes, wscale, col_scale, save, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}

extern "C" int smpq_trial_rows_patch(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                                     const int32_t* bits, int n, int semantics, int wlimbs, const float* bn_a,
                                     int8_t* codes, int8_t* codes_km, float* wscale, float* col_scale, void* save,
                                     int32_t* status, smpq_stream_t stream) {
  std::string err;
  const int rc = trial_rows_check(w, cout, cin, kh, kw, channels, bits, n, semantics, wlimbs, bn_a, codes, wscale,
                                  col_scale, save, status, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  const long long slot = SMPQ_TRIAL_SAVE_HEADER + (long long)wlimbs * cin * kh * kw;
  hipLaunchKernelGGL(trial_rows_patch_kernel, dim3(n), dim3(kQThreads), 0, (hipStream_t)stream, w, cout, cin, kh * kw,
                     channels, bits, semantics, wlimbs, bn_a, codes, codes_km, wscale, col_scale,
                     static_cast<int8_t*>(save), slot, status);
  return check_hip(hipGetLastError(), "trial_rows_patch_kernel launch");
}

extern "C" int smpq_trial_rows_restore(int cout, int K, const int32_t* channels, int n, int wlimbs, int8_t* codes,
                                       int8_t* codes_km, float* wscale, float* col_scale, const void* save,
                                       smpq_stream_t stream) {
  std::string err;
  const int rc = trial_rows_restore_check(cout, K, channels, n, wlimbs, codes, wscale, col_scale, save, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  const long long slot = SMPQ_TRIAL_SAVE_HEADER + (long long)wlimbs * K;
  hipLaunchKernelGGL(trial_rows_restore_kernel, dim3(n), dim3(kQThreads), 0, (hipStream_t)stream, cout, K, channels,
                     wlimbs, codes, codes_km, wscale, col_scale, static_cast<const int8_t*>(save), slot);
  return check_hip(hipGetLastError(), "trial_rows_restore_kernel launch");
}

extern "C" int smpq_trial_rows_patch_host(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                                          const int32_t* bits, int n, int semantics, int wlimbs, const float* bn_a,
                                          int8_t* codes, float* wscale, float* col_scale, void* save,
                                          int32_t* status) {
  std::string err;
  const int rc = trial_rows_patch_host(w, cout, cin, kh, kw, channels, bits, n, semantics, wlimbs, bn_a, codes, wscale,
                                       col_scale, save, status, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}

extern "C" int smpq_trial_rows_restore_host(int cout, int K, const int32_t* channels, int n, int wlimbs,
                                            int8_t* codes, float* wscale, float* col_scale, const void* save) {
  std::string err;
  const int rc = trial_rows_restore_host(cout, K, channels, n, wlimbs, codes, wscale, col_scale, save, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}

extern "C" int smpq_trial_rows_patch_x8(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                                        const int32_t* bits, int n, int semantics, const float* bn_a, int8_t* codes,
                                        int8_t* codes_km, int32_t* offset, float* wscale, float* col_scale, void* save,
                                        int32_t* status, smpq_stream_t stream) {
  std::string err;
  const int rc = trial_rows_x8_check("smpq_trial_rows_patch_x8", w, cout, cin, kh, kw, channels, bits, n, semantics,
                                     bn_a, codes, wscale, col_scale, save, status, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  const long long slot = SMPQ_TRIAL_SAVE_HEADER + (long long)cin * kh * kw;
  hipLaunchKernelGGL(trial_rows_patch_x8_kernel, dim3(n), dim3(kQThreads), 0, (hipStream_t)stream, w, cout, cin,
                     kh * kw, channels, bits, semantics, bn_a, codes, codes_km, offset, wscale, col_scale,
                     static_cast<int8_t*>(save), slot, status);
  return check_hip(hipGetLastError(), "trial_rows_patch_x8_kernel launch");
}

extern "C" int smpq_trial_rows_restore_x8(int cout, int K, const int32_t* channels, int n, int8_t* codes,
                                          int8_t* codes_km, int32_t* offset, float* wscale, float* col_scale,
                                          const void* save, smpq_stream_t stream) {
  std::string err;
  const int rc = trial_rows_restore_x8_check("smpq_trial_rows_restore_x8", cout, K, channels, n, codes, wscale,
                                             col_scale, save, &err);
  if (rc != SMPQ_OK) return fail(rc, err);
  const long long slot = SMPQ_TRIAL_SAVE_HEADER + (long long)K;
  hipLaunchKernelGGL(trial_rows_restore_x8_kernel, dim3(n), dim3(kQThreads), 0, (hipStream_t)stream, cout, K, channels,
                     codes, codes_km, offset, wscale, col_scale, static_cast<const int8_t*>(save), slot);
  return check_hip(hipGetLastError(), "trial_rows_restore_x8_kernel launch");
}

extern "C" int smpq_trial_rows_patch_x8_host(const float* w, int cout, int cin, int kh, int kw,
                                             const int32_t* channels, const int32_t* bits, int n, int semantics,
                                             const float* bn_a, int8_t* codes, int32_t* offset, float* wscale,
                                             float* col_scale, void* save, int32_t* status) {
  std::string err;
  const int rc = trial_rows_patch_x8_host(w, cout, cin, kh, kw, channels, bits, n, semantics, bn_a, codes, offset,
                                          wscale, col_scale, save, status, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}

extern "C" int smpq_trial_rows_restore_x8_host(int cout, int K, const int32_t* channels, int n, int8_t* codes,
                                               int32_t* offset, float* wscale, float* col_scale, const void* save) {
  std::string err;
  const int rc = trial_rows_restore_x8_host(cout, K, channels, n, codes, offset, wscale, col_scale, save, &err);
  return rc != SMPQ_OK ? fail(rc, err) : rc;
}
