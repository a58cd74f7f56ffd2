// uint8 <-> fp32 through a per-channel 256-entry table (include/smpq.h has the normative text):
// the resident evaluation set (smpq/batches.py ResidentSet) keeps Resize / CenterCrop / ToTensor /
// Normalize images as the uint8 they came from and replays them bit for bit. Values are LOOKED UP,
// never recomputed: a fused multiply-add restatement of (u / 255 - mean) / std differs from torch's
// three rounded operators in most of the 768 entries.
//
// Work is cut into tiles of one channel plane [hw] x 4096 elements, so the table row is uniform in
// a tile and nothing ever straddles two planes. The table (at most 4 KB) is staged in LDS once per
// workgroup; workgroups walk the tiles with a grid stride.
//   decode, vector form   a lane loads 16 B of u; the wave's 1 KiB of u is transposed through LDS
//                         so that each of its four 16-B store instructions writes 1 KiB of
//                         consecutive x (a lane storing its own 64 B, four stores 16 B apart, ran
//                         at 0.6 of this form's rate). A plane starts at an
//                         arbitrary byte, so each plane peels a head (up to the first 16-B aligned
//                         byte of u) and a tail (< 16 elements), both scalar. The 16-B alignment of
//                         the x stores follows from that of the u loads exactly when
//                         (x_addr / 4 - u_addr) % 4 == 0, which does not depend on the plane:
//                         the entry point checks it once and otherwise launches the
//   decode, scalar form   one element per lane and step (coalesced 1-B loads, 4-B stores).
//   encode                one element per lane and step: binary search of the row (8 steps), the
//                         off-grid count reduced over the wave and the workgroup, one atomic per
//                         workgroup. Runs only while the cache is filled.
// Plain (temporal) stores throughout: the engine's absmax / input-quantize kernels read x next.
#include <cmath>
#include <cstring>

#include "common.h"

namespace smpq {

constexpr int kU8Threads = 256;
constexpr int kU8Waves = kU8Threads / kWave;
constexpr int kU8Vec = 16;                        // elements per lane and step in the vector form
constexpr int kU8Tile = kU8Threads * kU8Vec;      // elements of a plane per tile
constexpr int kU8MaxC = 4;
constexpr int kU8MaxGrid = 2048;                  // 256 CUs x 8 resident workgroups

// largest v with row[v] <= x, 0 when there is none or x is NaN
__host__ __device__ inline int u8lut_search(const float* row, float x) {
  if (!(x >= row[0])) return 0;
  int lo = 0, hi = 255;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void u8lut_stage(float* s_lut, const float* __restrict__ lut, int c) {
  for (int i = threadIdx.x; i < c * 256; i += kU8Threads) s_lut[i] = lut[i];
  __syncthreads();
}

template <bool kVector>
__global__ __launch_bounds__(kU8Threads) void u8lut_decode_kernel(
    const uint8_t* __restrict__ u, int c, int hw, const float* __restrict__ lut, float* __restrict__ x,
    int tiles_per_plane, long long tiles) {
  __shared__ float s_lut[kU8MaxC * 256];
  __shared__ uint32_t s_words[kVector ? kU8Waves : 1][4 * kWave];  // per wave: 64 groups of 16 B
  u8lut_stage(s_lut, lut, c);
  const int tid = threadIdx.x;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {  // (block-uniform: barriers inside are safe)
    const int plane = (int)(t / tiles_per_plane);
    const int chunk = (int)(t - (long long)plane * tiles_per_plane);
    const float* row = s_lut + (plane % c) * 256;
    const uint8_t* up = u + (size_t)plane * hw;
    float* xp = x + (size_t)plane * hw;
    if (kVector) {
      // head: up to the first 16-B aligned byte of this plane's u (x is 16-B aligned there too)
      const int head = min(hw, (int)((16u - (unsigned)((uintptr_t)up & 15u)) & 15u));
      const int groups = (hw - head) / kU8Vec;
      if (chunk == 0) {
        const int tail0 = head + groups * kU8Vec;  // tail: fewer than 16 elements
        if (tid < head) xp[tid] = row[up[tid]];
        if (tid < hw - tail0) xp[tail0 + tid] = row[up[tail0 + tid]];
      }
      // body: a lane loads the 16 B of one group; the wave's 64 groups (256 words) pass through
      // its own LDS slab so that lane l then owns words l, 64 + l, 128 + l, 192 + l and every store
      // instruction of the wave writes 1 KiB of consecutive x
      const int wave = tid / kWave, lane = tid % kWave;
      const int g0 = chunk * kU8Threads + wave * kWave;  // the wave's first group
      if (g0 + lane < groups)
        *reinterpret_cast<uint4*>(&s_words[wave][4 * lane]) =
            *reinterpret_cast<const uint4*>(up + head + (g0 + lane) * kU8Vec);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = j * kWave + lane;  // word q of the slab = elements 4q .. 4q + 3 of the wave's run
        if (g0 + q / 4 < groups) {
          const uint32_t w = s_words[wave][q];
          v4i v;
          v.x = __float_as_int(row[w & 255u]);
          v.y = __float_as_int(row[(w >> 8) & 255u]);
          v.z = __float_as_int(row[(w >> 16) & 255u]);
          v.w = __float_as_int(row[w >> 24]);
          st16(xp + head + g0 * kU8Vec + 4 * q, v);
        }
      }
      __syncthreads();  // the slab is rewritten by the next tile
    } else {
      const int e0 = chunk * kU8Tile;
      const int len = min(kU8Tile, hw - e0);
      for (int i = tid; i < len; i += kU8Threads) xp[e0 + i] = row[up[e0 + i]];
    }
  }
}

__global__ __launch_bounds__(kU8Threads) void u8lut_encode_kernel(
    const float* __restrict__ x, int c, int hw, const float* __restrict__ lut, uint8_t* __restrict__ u,
    uint32_t* __restrict__ bad, int tiles_per_plane, long long tiles) {
  __shared__ float s_lut[kU8MaxC * 256];
  __shared__ int s_bad[kU8Waves];
  u8lut_stage(s_lut, lut, c);
  const int tid = threadIdx.x;
  int off = 0;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int plane = (int)(t / tiles_per_plane);
    const int chunk = (int)(t - (long long)plane * tiles_per_plane);
    const float* row = s_lut + (plane % c) * 256;
    const float* xp = x + (size_t)plane * hw;
    uint8_t* up = u + (size_t)plane * hw;
    const int e0 = chunk * kU8Tile;
    const int len = min(kU8Tile, hw - e0);
    for (int i = tid; i < len; i += kU8Threads) {
      const float v = xp[e0 + i];
      const int code = u8lut_search(row, v);
      up[e0 + i] = (uint8_t)code;
      off += __float_as_uint(row[code]) != __float_as_uint(v);
    }
  }
  off = wave_sum_i(off);
  if (tid % kWave == 0) s_bad[tid / kWave] = off;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int i = 0; i < kU8Waves; ++i) total += s_bad[i];
    if (total) atomicAdd(bad, (uint32_t)total);
  }
}

}  // namespace smpq

using namespace smpq;

// n, c, hw >= 1, c <= 4, n * c * hw < 2^31
static int u8lut_shape_ok(const char* what, int n, int c, int hw) {
  if (n < 1 || c < 1 || c > kU8MaxC || hw < 1 || (long long)n * c * hw >= (1ll << 31))
    return fail(SMPQ_E_SHAPE, std::string(what) + ": need n, hw >= 1, 1 <= c <= 4 and n * c * hw < 2^31");
  return SMPQ_OK;
}

static int u8lut_table_ok(const char* what, const float* lut, int c) {
  for (int ch = 0; ch < c; ++ch)
    for (int v = 0; v < 256; ++v) {
      const float a = lut[ch * 256 + v];
      if (!(std::fabs(a) <= 3.402823466e+38f) || (v && !(lut[ch * 256 + v - 1] < a)))
        return fail(SMPQ_E_INVALID, std::string(what) + ": table row not finite and strictly increasing");
    }
  return SMPQ_OK;
}

static void u8lut_grid(int n, int c, int hw, int* tiles_per_plane, long long* tiles, int* grid) {
  *tiles_per_plane = (hw - 1) / kU8Tile + 1;
  *tiles = (long long)n * c * *tiles_per_plane;
  *grid = (int)(*tiles < kU8MaxGrid ? *tiles : kU8MaxGrid);
}

extern "C" int smpq_u8lut_decode(const uint8_t* u, int n, int c, int hw, const float* lut, float* x,
                                 smpq_stream_t stream) {
  if (!u || !lut || !x || ((uintptr_t)x & 3u)) return fail(SMPQ_E_INVALID, "smpq_u8lut_decode: bad arguments");
  if (int rc = u8lut_shape_ok("smpq_u8lut_decode", n, c, hw)) return rc;
  int tpp, grid;
  long long tiles;
  u8lut_grid(n, c, hw, &tpp, &tiles, &grid);
  // the 16-B stores of x are aligned wherever the 16-B loads of u are (see the head of this file)
  const bool vec = ((((uintptr_t)x >> 2) - (uintptr_t)u) & 3u) == 0;
  if (vec)
    hipLaunchKernelGGL(u8lut_decode_kernel<true>, dim3(grid), dim3(kU8Threads), 0, (hipStream_t)stream, u, c, hw,
                       lut, x, tpp, tiles);
  else
    hipLaunchKernelGGL(u8lut_decode_kernel<false>, dim3(grid), dim3(kU8Threads), 0, (hipStream_t)stream, u, c, hw,
                       lut, x, tpp, tiles);
  return check_hip(hipGetLastError(), "u8lut_decode_kernel launch");
}

extern "C" int smpq_u8lut_encode(const float* x, int n, int c, int hw, const float* lut, uint8_t* u, uint32_t* bad,
                                 smpq_stream_t stream) {
  if (!x || !lut || !u || !bad || ((uintptr_t)x & 3u) || ((uintptr_t)bad & 3u))
    return fail(SMPQ_E_INVALID, "smpq_u8lut_encode: bad arguments");
  if (int rc = u8lut_shape_ok("smpq_u8lut_encode", n, c, hw)) return rc;
  int tpp, grid;
  long long tiles;
  u8lut_grid(n, c, hw, &tpp, &tiles, &grid);
  hipLaunchKernelGGL(u8lut_encode_kernel, dim3(grid), dim3(kU8Threads), 0, (hipStream_t)stream, x, c, hw, lut, u,
                     bad, tpp, tiles);
  return check_hip(hipGetLastError(), "u8lut_encode_kernel launch");
}

// ------------------------------------------------------------------------------------------
// host twins (native C++, same semantics; they also validate the table)
// ------------------------------------------------------------------------------------------
extern "C" int smpq_u8lut_decode_host(const uint8_t* u, int n, int c, int hw, const float* lut, float* x) {
  if (!u || !lut || !x) return fail(SMPQ_E_INVALID, "smpq_u8lut_decode_host: bad arguments");
  if (int rc = u8lut_shape_ok("smpq_u8lut_decode_host", n, c, hw)) return rc;
  if (int rc = u8lut_table_ok("smpq_u8lut_decode_host", lut, c)) return rc;
  for (int p = 0; p < n * c; ++p) {
    const float* row = lut + (p % c) * 256;
    const uint8_t* up = u + (size_t)p * hw;
    float* xp = x + (size_t)p * hw;
    for (int e = 0; e < hw; ++e) xp[e] = row[up[e]];
  }
  return SMPQ_OK;
}

extern "C" int smpq_u8lut_encode_host(const float* x, int n, int c, int hw, const float* lut, uint8_t* u,
                                      uint32_t* bad) {
  if (!x || !lut || !u || !bad) return fail(SMPQ_E_INVALID, "smpq_u8lut_encode_host: bad arguments");
  if (int rc = u8lut_shape_ok("smpq_u8lut_encode_host", n, c, hw)) return rc;
  if (int rc = u8lut_table_ok("smpq_u8lut_encode_host", lut, c)) return rc;
  uint32_t off = 0;
  for (int p = 0; p < n * c; ++p) {
    const float* row = lut + (p % c) * 256;
    const float* xp = x + (size_t)p * hw;
    uint8_t* up = u + (size_t)p * hw;
    for (int e = 0; e < hw; ++e) {
      const int code = u8lut_search(row, xp[e]);
      up[e] = (uint8_t)code;
      off += std::memcmp(&row[code], &xp[e], 4) != 0;
    }
  }
  *bad += off;
  return SMPQ_OK;
}
