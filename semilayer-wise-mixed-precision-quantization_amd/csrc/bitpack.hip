// Bit-packed weight store, format smpq-packed/1 (include/smpq.h has the normative description):
// plan / store / load of one fp32 weight [cout][k] whose quantized channels are kept as b-bit
// codes u = m - base in a little-endian bit stream of 32-bit words, every other channel as its
// IEEE bit patterns. Unpacking recomputes fl32((float)(base + u) * step): bitwise the original,
// because a channel is packed only when the planner has verified exactly that product for every
// value. FP contraction is off (one rounded multiply, as the quantizer's own functions.py:41).
//
// One workgroup per output channel in all three kernels (channels are at most 4608 elements,
// see quant.hip): the per-channel scalars (mode, base, step, word offset) are uniform in a block.
//   plan   one pass over the channel + wave64 reductions, as pack_weights_ex_kernel
//   store  a thread owns whole 32-bit words and gathers the (up to 32) codes overlapping each:
//          no atomics, every planned word written exactly once, nothing else written
//   load   a thread owns elements; it reads the word holding the code's first bit, and the next
//          word only when the code straddles it (which is then inside the channel's own words)
#include <cmath>
#include <cstring>

#include "common.h"

#pragma clang fp contract(off)

namespace smpq {

constexpr int kBpThreads = 256;
constexpr int kBpWaves = kBpThreads / kWave;
constexpr float kBpCodeMax = 8388608.f;  // 2^23: |m| up to here converts to int and back exactly
constexpr int kBpMaxK = 1 << 26;         // k * 8 bits stays inside int32

// Conditions 3-5 of the format for one value: finite, |m| <= 2^23, fl32((float)m * step) == v
// bitwise. The product is formed from the INTEGER code, as the unpacker forms it: a -0.0 weight
// (m = 0 gives +0.0) is therefore off-grid and sends its channel to the raw form.
__host__ __device__ inline bool bp_code(float v, float s, int* m_out) {
#ifdef __HIP_DEVICE_COMPILE__
  const float mf = rintf(__fdiv_rn(v, s));
#else
  const float mf = std::nearbyintf(v / s);
#endif
  if (!(fabsf(v) <= 3.402823466e+38f) || !(fabsf(mf) <= kBpCodeMax)) return false;
  const int m = (int)mf;
#ifdef __HIP_DEVICE_COMPILE__
  const float back = __fmul_rn((float)m, s);
  const bool same = __float_as_uint(back) == __float_as_uint(v);
#else
  const float back = (float)m * s;
  uint32_t a, b;
  std::memcpy(&a, &back, 4);
  std::memcpy(&b, &v, 4);
  const bool same = a == b;
#endif
  *m_out = m;
  return same;
}

__host__ __device__ inline bool bp_step_ok(int b, float s) {
  return b >= 1 && b <= 8 && s > 0.f && s <= 3.402823466e+38f;  // conditions 1-2 (NaN fails both)
}

__host__ __device__ inline int bp_words(int k, int b) { return (k * b + 31) >> 5; }

__global__ __launch_bounds__(kBpThreads) void bitpack_plan_kernel(
    const float* __restrict__ w, int k, const int8_t* __restrict__ qbits, const float* __restrict__ step,
    int8_t* __restrict__ mode, int32_t* __restrict__ base, int32_t* __restrict__ words) {
  __shared__ int smem[3 * kBpWaves];
  const int c = blockIdx.x;
  const int b = qbits[c];
  const float s = step[c];
  const float* row = w + (size_t)c * k;
  int bad = bp_step_ok(b, s) ? 0 : 1;
  int mmin = INT32_MAX, mmax = INT32_MIN;
  if (!bad) {
    for (int i = threadIdx.x; i < k; i += kBpThreads) {
      int m;
      if (!bp_code(row[i], s, &m)) {
        bad = 1;
        break;
      }
      mmin = min(mmin, m);
      mmax = max(mmax, m);
    }
  }
  mmin = wave_min_i(mmin);
  mmax = wave_max_i(mmax);
  bad = wave_max_i(bad);
  const int wid = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    smem[wid] = mmin;
    smem[kBpWaves + wid] = mmax;
    smem[2 * kBpWaves + wid] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mmin = smem[0], mmax = smem[kBpWaves], bad = smem[2 * kBpWaves];
    for (int i = 1; i < kBpWaves; ++i) {
      mmin = min(mmin, smem[i]);
      mmax = max(mmax, smem[kBpWaves + i]);
      bad |= smem[2 * kBpWaves + i];
    }
    // condition 6; with bad == 0 every thread of a k >= 1 channel saw a code, |m| <= 2^23
    const bool packed = !bad && (mmax - mmin) <= (1 << b) - 1;
    mode[c] = packed ? (int8_t)b : (int8_t)0;
    base[c] = packed ? mmin : 0;
    words[c] = packed ? bp_words(k, b) : k;
  }
}

__global__ __launch_bounds__(kBpThreads) void bitpack_store_kernel(
    const float* __restrict__ w, int k, const int8_t* __restrict__ mode, const int32_t* __restrict__ base,
    const float* __restrict__ step, const int64_t* __restrict__ word_off, uint32_t* __restrict__ payload) {
  const int c = blockIdx.x;
  const int b = mode[c];
  const float* row = w + (size_t)c * k;
  uint32_t* out = payload + word_off[c];
  if (b <= 0 || b > 8) {  // raw: the bit patterns
    for (int i = threadIdx.x; i < k; i += kBpThreads) out[i] = __float_as_uint(row[i]);
    return;
  }
  const float s = step[c];
  const int m0 = base[c];
  const int nwords = bp_words(k, b);
  for (int wd = threadIdx.x; wd < nwords; wd += kBpThreads) {
    const int bit0 = wd * 32;
    const int i0 = bit0 / b;                       // first code with a bit in this word
    const int i1 = min(k - 1, (bit0 + 31) / b);    // last one
    uint32_t word = 0;
    for (int i = i0; i <= i1; ++i) {
      const uint32_t u = (uint32_t)((int)rintf(__fdiv_rn(row[i], s)) - m0);
      const int sh = i * b - bit0;  // in (-b, 32)
      word |= sh >= 0 ? u << sh : u >> -sh;
    }
    out[wd] = word;
  }
}

__global__ __launch_bounds__(kBpThreads) void bitpack_load_kernel(
    const uint32_t* __restrict__ payload, int k, const int8_t* __restrict__ mode,
    const int32_t* __restrict__ base, const float* __restrict__ step, const int64_t* __restrict__ word_off,
    float* __restrict__ w) {
  const int c = blockIdx.x;
  const int b = mode[c];
  float* row = w + (size_t)c * k;
  const uint32_t* in = payload + word_off[c];
  if (b <= 0 || b > 8) {
    for (int i = threadIdx.x; i < k; i += kBpThreads) row[i] = __uint_as_float(in[i]);
    return;
  }
  const float s = step[c];
  const int m0 = base[c];
  const uint32_t mask = (1u << b) - 1u;
  for (int i = threadIdx.x; i < k; i += kBpThreads) {
    const int bit = i * b;
    const int w0 = bit >> 5, sh = bit & 31;
    uint32_t u = in[w0] >> sh;
    if (sh + b > 32) u |= in[w0 + 1] << (32 - sh);  // sh > 0 here; the word is the channel's own
    row[i] = __fmul_rn((float)(m0 + (int)(u & mask)), s);
  }
}

}  // namespace smpq

using namespace smpq;

static int bp_args_ok(const char* what, int cout, int k) {
  if (cout <= 0 || k <= 0) return fail(SMPQ_E_INVALID, std::string(what) + ": bad arguments");
  if (k > kBpMaxK) return fail(SMPQ_E_SHAPE, std::string(what) + ": k above 2^26");
  return SMPQ_OK;
}

extern "C" int smpq_bitpack_plan(const float* w, int cout, int k, const int8_t* qbits, const float* step,
                                 int8_t* mode, int32_t* base, int32_t* words, smpq_stream_t stream) {
  if (!w || !qbits || !step || !mode || !base || !words) return fail(SMPQ_E_INVALID, "smpq_bitpack_plan: bad arguments");
  if (int rc = bp_args_ok("smpq_bitpack_plan", cout, k)) return rc;
  hipLaunchKernelGGL(bitpack_plan_kernel, dim3(cout), dim3(kBpThreads), 0, (hipStream_t)stream, w, k, qbits, step,
                     mode, base, words);
  return check_hip(hipGetLastError(), "bitpack_plan_kernel launch");
}

extern "C" int smpq_bitpack_store(const float* w, int cout, int k, const int8_t* mode, const int32_t* base,
                                  const float* step, const int64_t* word_off, uint32_t* payload,
                                  smpq_stream_t stream) {
  if (!w || !mode || !base || !step || !word_off || !payload)
    return fail(SMPQ_E_INVALID, "smpq_bitpack_store: bad arguments");
  if (int rc = bp_args_ok("smpq_bitpack_store", cout, k)) return rc;
  hipLaunchKernelGGL(bitpack_store_kernel, dim3(cout), dim3(kBpThreads), 0, (hipStream_t)stream, w, k, mode, base,
                     step, word_off, payload);
  return check_hip(hipGetLastError(), "bitpack_store_kernel launch");
}

extern "C" int smpq_bitpack_load(const uint32_t* payload, int cout, int k, const int8_t* mode, const int32_t* base,
                                 const float* step, const int64_t* word_off, float* w, smpq_stream_t stream) {
  if (!payload || !mode || !base || !step || !word_off || !w)
    return fail(SMPQ_E_INVALID, "smpq_bitpack_load: bad arguments");
  if (int rc = bp_args_ok("smpq_bitpack_load", cout, k)) return rc;
  hipLaunchKernelGGL(bitpack_load_kernel, dim3(cout), dim3(kBpThreads), 0, (hipStream_t)stream, payload, k, mode,
                     base, step, word_off, w);
  return check_hip(hipGetLastError(), "bitpack_load_kernel launch");
}

// ------------------------------------------------------------------------------------------
// host twins (native C++, same arithmetic)
// ------------------------------------------------------------------------------------------
extern "C" int smpq_bitpack_plan_host(const float* w, int cout, int k, const int8_t* qbits, const float* step,
                                      int8_t* mode, int32_t* base, int32_t* words) {
  if (!w || !qbits || !step || !mode || !base || !words)
    return fail(SMPQ_E_INVALID, "smpq_bitpack_plan_host: bad arguments");
  if (int rc = bp_args_ok("smpq_bitpack_plan_host", cout, k)) return rc;
  for (int c = 0; c < cout; ++c) {
    const int b = qbits[c];
    const float s = step[c];
    const float* row = w + (size_t)c * k;
    bool ok = bp_step_ok(b, s);
    int mmin = INT32_MAX, mmax = INT32_MIN;
    for (int i = 0; ok && i < k; ++i) {
      int m;
      ok = bp_code(row[i], s, &m);
      if (ok) {
        mmin = m < mmin ? m : mmin;
        mmax = m > mmax ? m : mmax;
      }
    }
    const bool packed = ok && (mmax - mmin) <= (1 << b) - 1;
    mode[c] = packed ? (int8_t)b : (int8_t)0;
    base[c] = packed ? mmin : 0;
    words[c] = packed ? bp_words(k, b) : k;
  }
  return SMPQ_OK;
}

extern "C" int smpq_bitpack_store_host(const float* w, int cout, int k, const int8_t* mode, const int32_t* base,
                                       const float* step, const int64_t* word_off, uint32_t* payload) {
  if (!w || !mode || !base || !step || !word_off || !payload)
    return fail(SMPQ_E_INVALID, "smpq_bitpack_store_host: bad arguments");
  if (int rc = bp_args_ok("smpq_bitpack_store_host", cout, k)) return rc;
  for (int c = 0; c < cout; ++c) {
    const int b = mode[c];
    const float* row = w + (size_t)c * k;
    uint32_t* out = payload + word_off[c];
    if (b <= 0 || b > 8) {
      std::memcpy(out, row, (size_t)k * 4);
      continue;
    }
    const float s = step[c];
    const int nwords = bp_words(k, b);
    for (int wd = 0; wd < nwords; ++wd) out[wd] = 0;
    for (int i = 0; i < k; ++i) {
      const uint32_t u = (uint32_t)((int)std::nearbyintf(row[i] / s) - base[c]);
      const int bit = i * b, w0 = bit >> 5, sh = bit & 31;
      out[w0] |= u << sh;
      if (sh + b > 32) out[w0 + 1] |= u >> (32 - sh);
    }
  }
  return SMPQ_OK;
}

extern "C" int smpq_bitpack_load_host(const uint32_t* payload, int cout, int k, const int8_t* mode,
                                      const int32_t* base, const float* step, const int64_t* word_off, float* w) {
  if (!payload || !mode || !base || !step || !word_off || !w)
    return fail(SMPQ_E_INVALID, "smpq_bitpack_load_host: bad arguments");
  if (int rc = bp_args_ok("smpq_bitpack_load_host", cout, k)) return rc;
  for (int c = 0; c < cout; ++c) {
    const int b = mode[c];
    float* row = w + (size_t)c * k;
    const uint32_t* in = payload + word_off[c];
    if (b <= 0 || b > 8) {
      std::memcpy(row, in, (size_t)k * 4);
      continue;
    }
    const float s = step[c];
    const uint32_t mask = (1u << b) - 1u;
    for (int i = 0; i < k; ++i) {
      const int bit = i * b, w0 = bit >> 5, sh = bit & 31;
      uint32_t u = in[w0] >> sh;
      if (sh + b > 32) u |= in[w0 + 1] << (32 - sh);
      row[i] = (float)(base[c] + (int)(u & mask)) * s;
    }
  }
  return SMPQ_OK;
}
