// Shared by the two quantized-conv kernels (conv.hip: register-staged, any cin; conv_glds.hip:
// LDS-DMA staged, cin % 64 == 0). Not part of the public ABI.
#pragma once

#include <map>
#include <mutex>
#include <tuple>

#include "common.h"

namespace smpq {

constexpr int kKStep = 64;  // K per MFMA (i8 16x16x64)

struct ConvArgs {
  const int8_t* xq;       // [L][n][h][w][cin] activation limb planes
  long long plane;        // elements per activation plane
  const float* x_absmax;  // [n]
  const int8_t* codes;    // [LW][cout][K] weight limb planes
  long long wplane;       // elements per weight plane (cout*K)
  const int32_t* w_off;   // [cout] (LW == 1 only) or NULL
  const float* col_scale;
  const float* col_shift;
  const float* residual;  // fp32 NHWC residual, or NULL
  const int8_t* res_q;    // [L][M][cout] residual limb planes (static range), or NULL
  float res_scale;        // residual value = res_scale * sum_l 256^l digit_l
  float* y;               // fp32 NHWC output, or NULL
  float* y_absmax;
  int8_t* yq;             // [L][M][cout] output limb planes (static range), or NULL
  float yq_inv;           // QMAX / range of the output quantizer
  int32_t* overflow;      // set to 1 when |y| exceeded the static range (then clamped)
  int n, h, w, cin, cout, kh, kw, stride, pad, ho, wo;
  int M, K, ksteps, cchunks;
  int relu, has_offset;
  int nt_store;  // limb-plane output stores with the non-temporal policy (outputs too big for the MALL)
  // x / d = (x * mul) >> shr for 0 <= x < 2^31 (fast_div_init): output pixels per image, output
  // width, and (set by the tile launcher) channel tiles
  unsigned hw_mul, wo_mul, ntc_mul;
  int hw_shr, wo_shr, ntc_shr;
  float inv_qmax;
  int s2d;  // space-to-depth stem (smpq_stem_conv_s2d_q): cin 16, 4 x 4 taps, K step = one tap row
  // codes in the K-major layout [LW][K/64][cout][64] (smpq_conv2d_fwd_q_km; LDS-DMA kernel only):
  // the 64-B K slices of 16 consecutive output channels are one contiguous KiB, so every weight
  // DMA piece is whole cache lines instead of 16 half lines
  int w_kmajor;
};

// Division by a runtime constant d >= 1 for numerators in [0, 2^31): p = 31 + ceil(log2 d),
// mul = ceil(2^p / d) (< 2^32), x / d == (x * mul) >> p. Two instructions instead of the ~20 of a
// generic 32-bit division (the conv prologues decompose pixel indices with it).
inline void fast_div_init(int d, unsigned& mul, int& shr) {
  int l = 0;
  while ((1LL << l) < (long long)d) ++l;
  shr = 31 + l;
  mul = (unsigned)(((1ULL << shr) + (unsigned long long)d - 1) / (unsigned long long)d);
}
__device__ __forceinline__ int fast_div(int x, unsigned mul, int shr) {
  return (int)(((unsigned long long)(unsigned)x * mul) >> shr);
}

template <int L>
__device__ __host__ constexpr float act_qmax() {
  return L == 1 ? 127.f : (L == 2 ? 32512.f : 8323072.f);
}

// The activation quantizers' scale for a per-image range am: code = rne((x * pre) * inv), clamped to
// +-QMAX. pre is 1 and inv = QMAX / am, except below 2^-64, where both sides are scaled by 2^64 first:
// QMAX / am passes FLT_MAX from am ~ 2.4e-32 at 3 limbs, and an infinite inv turns every zero
// activation into NaN and then, through the clamp, into -QMAX. Powers of two scale exactly, so every
// code that the unscaled form computed with a finite inv is unchanged.
struct ActScale {
  float pre, inv;
  __device__ __forceinline__ float operator()(float x) const { return (x * pre) * inv; }
};
template <int L>
__device__ __forceinline__ ActScale act_scale(float am) {
  const float pre = am < 0x1p-64f ? 0x1p64f : 1.f;
  return {pre, am > 0.f ? act_qmax<L>() / (am * pre) : 0.f};
}

// The (activation limb la, weight limb lw) passes every conv kernel keeps: those with
// la + lw >= limb_smin(L, LW) (the products of two low digits are below the output's resolution when
// both sides are wide); pass (la, lw) adds into int32 accumulator la + lw - SMIN of limb_nacc(L, LW),
// whose weight is 256^(la + lw). The one-row trial conv (trial_conv.hip) forms the same sums.
constexpr int limb_smin(int L, int LW) { return (L + LW - 4) > 0 ? (L + LW - 4) : 0; }
constexpr int limb_nacc(int L, int LW) { return L + LW - 1 - limb_smin(L, LW); }

template <int L>
__device__ __forceinline__ void split_limbs(int q, int* d) {
  // balanced base-256 digits, each in [-128, 127]
#pragma unroll
  for (int l = 0; l < L - 1; ++l) {
    const int lo = ((q + 128) & 255) - 128;
    d[l] = lo;
    q = (q - lo) >> 8;
  }
  d[L - 1] = q;
}

// Epilogue arithmetic shared by both kernels, written with explicit rounding so that every tile
// configuration of either kernel produces bitwise-identical outputs (no compiler contraction).
// v = sum_s fl(acc_s) * 256^(SMIN+s), accumulated in fp32 from the lowest limb weight up.
__device__ __forceinline__ float affine(float v, float rscale, float cscale, float cshift) {
  return __fmaf_rn(v, __fmul_rn(rscale, cscale), cshift);
}

// LDS-DMA staged kernel (conv_glds.hip)
int glds_num_cfgs();
void glds_cfg_info(int cfg, int* bm, int* bn, int* threads);
int glds_cfg_bk(int cfg);
bool glds_supported(int cfg, int cin, int cout, int kh, int kw, int limbs, int wlimbs);
int launch_glds(int cfg, int limbs, int wlimbs, const ConvArgs& a, hipStream_t s);
int glds_default_cfg(const ConvArgs& a, int limbs, int wlimbs);
bool glds_is_halo(int cfg);

// halo-patch 3x3 kernel (conv_halo.hip); its tile configs follow the LDS-DMA ones in the C-ABI's
// numbering (cfg = glds count + halo index)
int halo_num_cfgs();
void halo_cfg_info(int cfg, int* bm, int* bn, int* threads);
bool halo_supported(int cfg, int cin, int cout, int kh, int kw, int limbs, int wlimbs);
int launch_halo(int cfg, int limbs, int wlimbs, const ConvArgs& a, hipStream_t s);

// weight-stationary 1x1 tiles (conv_resident.hip); their configs follow the halo ones
int resident_num_cfgs();
void resident_cfg_info(int cfg, int* bm, int* bn, int* threads);
bool resident_supported(int cfg, int cin, int cout, int kh, int kw, int limbs, int wlimbs);
int launch_resident(int cfg, int limbs, int wlimbs, const ConvArgs& a, hipStream_t s);
bool glds_is_resident(int cfg);
// the same geometries with 3 weight limbs + ReLU (SMPQ_TILE_RESIDENT1X1_W); their configs come last
int resident_w_num_cfgs();
bool resident_w_supported(int cfg, int cin, int cout, int kh, int kw, int limbs, int wlimbs);
int launch_resident_w(int cfg, int limbs, int wlimbs, const ConvArgs& a, hipStream_t s);
bool glds_is_resident_w(int cfg);
// the Bottleneck tail chains: conv3 (+ fused downsample) (-> next conv1) (smpq_conv2d_chain_fwd)
bool resident_pair_supported(int cin, int cout1, int cout2, int limbs);
bool resident_chain_ds_supported(int cin, int cout1, int ds_cin, int ds_stride, int limbs);
// sg: slab groups per workgroup (1, or one resident_chain_sg_supported takes)
bool resident_chain_sg_supported(int cin, int cout1, int ds_cin, int ds_stride, int limbs, int offsets, int sg);
int launch_resident_chain(const ConvArgs& a, const ConvArgs* b, const ConvArgs* d, int limbs, int sg, hipStream_t s);
// the grid and the block -> (super-slab, first tile) order of a launch with slab groups
void resident_sg_map(int block, int blocks, int nss, int* sslab, int* tile0);
long long resident_sg_grid(long long budget, long long ntiles, int nss);

// grouped 3x3 kernels: conv_grouped.hip (a fragment span of 16, 32 or 64 input channels, the fragment's
// codes resident in registers) and conv_grouped_wide.hip (cin / groups and cout / groups multiples of
// 64, cin / groups >= 128: K streamed in 64-channel chunks). Both read the fragment-ordered copy of
// smpq_weights_grouped_expand.
struct GroupedArgs {
  const int8_t* xq;       // [3][n][h][w][cin]
  long long plane;        // bytes per activation limb plane
  const float* x_absmax;  // [n]
  const int8_t* wexp;     // [planes][nfrag][NK][64][16] fragment-ordered codes (+ indicator plane)
  const int32_t* w_off;   // [cout] or NULL
  const float* col_scale;
  const float* col_shift;
  float* y;
  float* y_absmax;
  int8_t* yq;
  int32_t* overflow;
  float yq_inv, inv_qmax;
  int n, h, w, cin, cout, ho, wo, cg, og, nfrag, relu;
  int ntw, tiles_img, tiles;
};
bool grouped_wide_shape(int cg, int og);
int launch_grouped_wide(const GroupedArgs& a, int wlimbs, int stride, bool lean, hipStream_t s);

// ---- narrow-channel geometry: conv_narrow.hip and conv_narrow_dilated.hip (K in 16-byte chunks over
// channel slabs, the fragment-ordered weight copy of smpq_weights_narrow_expand) ---------------------
constexpr int kNarrowTile = 8;               // output tile edge
constexpr int kNarrowLdsMax = 160 * 1024;    // LDS per workgroup on gfx950

struct NarrowGeo {
  int taps, pw;        // 9 or 1; patch edge in pixels
  int cs, nslab, cl;   // chunks per slab, slabs, chunks of the last slab
  int pp, rp;          // pixel and patch-row pitch in 16-B chunks
  int nkf, nk;         // MFMA steps of a full slab, of all slabs
  int lds_bytes;
};

// ds_read_b128 lane groups of gfx950 (tools/halo_conflicts.py): each is served in one pass when its 16
// addresses fall in 16 different 16-B slots mod 256 B
inline constexpr int kLaneGroups[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                           {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};

// chunk offset (16 B units) of a lane's fragment read: pixel fragment pf, K step j
__host__ __device__ inline int narrow_pix(int frow, int pf, int stride, int pp, int rp) {
  return stride * (2 * pf + (frow >> 3)) * rp + stride * (frow & 7) * pp;
}
__host__ __device__ inline int narrow_tap(int kk, int cwc, int taps, int pp, int rp) {
  const int tap = kk / cwc, sub = kk - tap * cwc;
  return tap < taps ? (tap / 3) * rp + (tap % 3) * pp + sub : 0;  // K padding: the codes are zero
}

// worst extra LDS cycles of one fragment read over all steps, pixel fragments and lane groups
inline int narrow_conflicts(int cwc, int taps, int stride, int pp, int rp) {
  int worst = 0;
  for (int j = 0; j < (taps * cwc + 3) / 4; ++j)
    for (int pf = 0; pf < 4; ++pf)
      for (int half = 0; half < 2; ++half)
        for (int g = 0; g < 2; ++g) {
          int chunk[16];
          for (int i = 0; i < 16; ++i) {
            const int lane = kLaneGroups[g][i] + 32 * half;
            chunk[i] = narrow_pix(lane & 15, pf, stride, pp, rp) + narrow_tap(4 * j + (lane >> 4), cwc, taps, pp, rp);
          }
          for (int b = 0; b < 16; ++b) {
            int distinct = 0;  // different chunks in bank slot b
            for (int q = 0; q < 16; ++q) {
              bool fresh = (chunk[q] & 15) == b;
              for (int r = 0; r < q; ++r) fresh = fresh && chunk[r] != chunk[q];
              distinct += fresh ? 1 : 0;
            }
            worst = distinct - 1 > worst ? distinct - 1 : worst;
          }
        }
  return worst;
}

inline int narrow_patch_bytes(int pw, int rp) { return (3 * pw * rp * 16 + 1023) / 1024 * 1024; }

// pitches of a slab of cwc chunks: of pixel pitches cwc .. cwc + 2 and up to 15 chunks of row padding,
// the pair with the fewest conflicts, then the smallest image; false when none fits LDS
inline bool narrow_pitch(int cwc, int taps, int stride, int pw, int& pp, int& rp) {
  int best = 1 << 30;
  for (int p = cwc; p < cwc + 3; ++p)
    for (int r = pw * p; r < pw * p + 16; ++r) {
      if (narrow_patch_bytes(pw, r) > kNarrowLdsMax) break;
      const int score = narrow_conflicts(cwc, taps, stride, p, r) * 65536 + r;
      if (score < best) best = score, pp = p, rp = r;
    }
  return best != (1 << 30);
}

// the slab walk, the LDS image and the step counts of (cin % 16 == 0, kh x kh, stride) (cached: the
// pitch search enumerates every fragment read)
inline bool narrow_geo(int cin, int kh, int stride, NarrowGeo& g) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, NarrowGeo> cache;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple(cin, kh, stride);
  const auto it = cache.find(key);
  if (it != cache.end()) {
    g = it->second;
    return g.cs > 0;
  }
  g = NarrowGeo{};
  g.taps = kh * kh;
  g.pw = kh == 1 ? kNarrowTile : stride * (kNarrowTile - 1) + 3;
  const int cc = cin / 16;
  for (int cwc = cc; cwc >= 1 && g.cs == 0; --cwc)
    if (narrow_patch_bytes(g.pw, g.pw * cwc) <= kNarrowLdsMax && narrow_pitch(cwc, g.taps, stride, g.pw, g.pp, g.rp))
      g.cs = cwc;
  if (g.cs > 0) {
    g.nslab = (cc + g.cs - 1) / g.cs;
    g.cl = cc - (g.nslab - 1) * g.cs;
    g.nkf = (g.taps * g.cs + 3) / 4;
    g.nk = (g.nslab - 1) * g.nkf + (g.taps * g.cl + 3) / 4;
    g.lds_bytes = narrow_patch_bytes(g.pw, g.rp);
  }
  cache[key] = g;
  return g.cs > 0;
}

inline long long narrow_expand_bytes(int wlimbs, int cout, const NarrowGeo& g) {
  return (long long)(wlimbs + (wlimbs == 1 ? 1 : 0)) * (cout / 16) * g.nk * 1024;
}

// the resident form's step count, or 0 for the streaming form
inline int narrow_resident_steps(const NarrowGeo& g) {
  return g.nslab == 1 && (g.nk == 1 || g.nk == 2 || g.nk == 3 || g.nk == 5 || g.nk == 7) ? g.nk : 0;
}

// one K step of the four pixel fragments: the lane's chunk at toff of the staged patch against the
// step's codes w[0 .. LW) (and the all-ones plane w[LW])
template <int LW, bool OFF, int NACC, int SMIN>
__device__ __forceinline__ void narrow_step(const int8_t* lds, int plimb, const int (&pixoff)[4], int toff,
                                            const v4i* w, v4i (&acc)[NACC][4], v4i (&gs)[OFF ? 3 : 1][4]) {
#pragma unroll
  for (int pf = 0; pf < 4; ++pf) {
    v4i fb[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) fb[l] = *reinterpret_cast<const v4i*>(lds + l * plimb + pixoff[pf] + toff);
#pragma unroll
    for (int la = 0; la < 3; ++la) {
#pragma unroll
      for (int lw = 0; lw < LW; ++lw)
        if (la + lw >= SMIN)
          acc[la + lw - SMIN][pf] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w[lw], fb[la], acc[la + lw - SMIN][pf], 0, 0, 0);
      if constexpr (OFF) gs[la][pf] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w[LW], fb[la], gs[la][pf], 0, 0, 0);
    }
  }
}

// The 4 codes (channels 0..3) held by one dword per limb plane, w[l] = the 4 balanced digits of
// limb l: q = sum_l d_l 256^l. With u_l = d_l + 128 (byte ^ 0x80) for the low limbs,
// q = sext24(u0 | u1 << 8 | d2 << 16) - 0x8080 (L = 3), sext16(u0 | d1 << 8) - 0x80 (L = 2).
template <int L>
__device__ __forceinline__ void decode4(const unsigned* w, int* q) {
  if constexpr (L == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = __builtin_amdgcn_sbfe((int)w[0], 8 * r, 8);
  } else if constexpr (L == 2) {
    const unsigned x0 = w[0] ^ 0x80808080u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned b = __builtin_amdgcn_perm(w[1], x0, (unsigned)r | ((unsigned)(r + 4) << 8) | 0x0c0c0000u);
      q[r] = __builtin_amdgcn_sbfe((int)b, 0, 16) - 0x80;
    }
  } else {
    const unsigned x0 = w[0] ^ 0x80808080u, x1 = w[1] ^ 0x80808080u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // [u0(2h), u1(2h), u0(2h+1), u1(2h+1)]
      const unsigned a = __builtin_amdgcn_perm(x1, x0, h == 0 ? 0x05010400u : 0x07030602u);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int r = 2 * h + e;
        const unsigned sel = (e == 0 ? 0x0100u : 0x0302u) | ((unsigned)(4 + r) << 16) | 0x0c000000u;
        const unsigned b = __builtin_amdgcn_perm(w[2], a, sel);
        q[r] = __mul24((int)b, 1) - 0x8080;  // 24-bit operand: sign from bit 23 (v_mad_i32_i24)
      }
    }
  }
}

// The digit dwords of 4 clamped codes (inverse of decode4): with Q = q + 0x8080 (L = 3) / q + 0x80
// (L = 2), digit l of q is byte l of Q, xor 0x80 for every limb below the top one.
template <int L>
__device__ __forceinline__ void encode4(const int* q, unsigned* w) {
  constexpr int bias = L == 3 ? 0x8080 : (L == 2 ? 0x80 : 0);
  const unsigned Q0 = (unsigned)(q[0] + bias), Q1 = (unsigned)(q[1] + bias), Q2 = (unsigned)(q[2] + bias),
                 Q3 = (unsigned)(q[3] + bias);
  const unsigned a = __builtin_amdgcn_perm(Q1, Q0, 0x05010400u);  // [Q0.b0, Q1.b0, Q0.b1, Q1.b1]
  const unsigned b = __builtin_amdgcn_perm(Q3, Q2, 0x05010400u);
  constexpr unsigned flip = 0x80808080u;
  w[0] = __builtin_amdgcn_perm(b, a, 0x05040100u) ^ (L > 1 ? flip : 0u);
  if constexpr (L >= 2) w[1] = __builtin_amdgcn_perm(b, a, 0x07060302u) ^ (L > 2 ? flip : 0u);
  if constexpr (L >= 3) {
    const unsigned c = __builtin_amdgcn_perm(Q1, Q0, 0x07030602u);  // [Q0.b2, Q1.b2, Q0.b3, Q1.b3]
    const unsigned d = __builtin_amdgcn_perm(Q3, Q2, 0x07030602u);
    w[2] = __builtin_amdgcn_perm(d, c, 0x05040100u);
  }
}

}  // namespace smpq
