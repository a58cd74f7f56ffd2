// 3x3 / stride 1 / pad 1 stem conv on <= 4 input channels (the conv1 of a CIFAR-style ResNet) for
// gfx950 on v_mfma_i32_16x16x64_i8, with its eval BatchNorm and ReLU folded in, on 3 activation limbs
// and 3 weight limbs (limb_smin(3, 3) / limb_nacc(3, 3): 6 MFMA passes into 3 int32 accumulator sets).
//
// Input planes. xq [3][n][h][w][4] int8: one dword per pixel and limb, channels c..3 zero
// (image_quantize_c4_kernel below: NCHW fp32 -> planes, the quantizer arithmetic of act_quantize_kernel).
//
// K order. [tap][4 channels]: 36 bytes, zero codes up to the 64 of ONE MFMA step. B lane
// (pixel = lane & 15, grp = lane >> 4) holds K bytes [16 grp, 16 grp + 16), i.e. taps 4 grp .. 4 grp + 3,
// one dword each, read from the staged patch. Group 2 carries tap 8 and three padding dwords, group 3
// padding only; the codes there are zero, so a padding lane re-reads the dword group 0 reads for the same
// register (tap t instead of 4 grp + t): inside LDS, and a broadcast of an address the read fetches anyway.
// The operand is the rows of smpq_pack_weights_grouped (cg = 4) zero-padded to 64 bytes: [3][cout][64].
//
// Work split. A workgroup is 4 waves and owns 64 output channels (blockIdx.x) and walks 8-row x 16-column
// output tiles: blockIdx.y, + gridDim.y, ... over the n * ceil(h / 8) * ceil(w / 16) tiles. Wave v owns
// tile rows 2 v and 2 v + 1: a pixel fragment is the 16 pixels of one tile row, and the wave runs it
// against all 64 channels, so one B fragment (3 limbs x 4 dword LDS reads) feeds 4 channel fragments x 6
// passes = 24 MFMAs. The weights of those, 4 fragments x 3 limbs x 1 step = 48 VGPRs, are loaded once per
// workgroup and stay in registers over every tile it walks.
//
// Halo patch in LDS, two stages. Per tile [limb][10 x 18 positions][4 B] = 2160 B. Thread i < 180 owns
// patch position i: while a tile is computed and stored, it holds the three limb dwords of the NEXT
// tile's position in registers (range-checked buffer loads issued before the MFMAs; a position outside
// the image, or a tile past the last, gets an out-of-range offset and loads zero), writes them to the
// other stage afterwards, and one barrier per tile hands the stages over.
// Bank conflicts (64 banks of 4 B, one ds_read_b32 of a wave = one pass when its dwords are in distinct
// banks): register t of the B fragment reads dword (row + ty) * 18 + pixel + tx with (ty, tx) the tap
// 4 grp + t, i.e. per lane group 16 consecutive dwords from base 18 ty + tx. The real groups' bases are
// t = 0: 0, 19, 38; t = 1: 1, 20; t = 2: 2, 36; t = 3: 18, 37 - the intervals [base, base + 16) are
// disjoint and span less than 64 dwords for every t, the padding groups repeat group 0's addresses, and
// a fragment's row only adds a constant: every fragment read is conflict-free at the natural pitch of
// 18, no padding or swizzle. The staging writes are lane-linear dwords.
//
// Epilogue: conv_common.h / lds_dma.h arithmetic (lean_quad, lean_v1, affine, encode4, transpose4), so
// a value is rounded as the dense kernels round it: the lean static-range form when only limb planes are
// wanted, the general form (fp32 y, y_absmax, optional limb planes) otherwise. A lane ends with channels
// 16 cf + 4 grp .. + 3 of its pixel for the four channel fragments cf; transpose4 over cf gives lane group
// g the pixel's channels 16 g .. 16 g + 15, one 16-B store per limb, the four groups 64 contiguous bytes
// (with cout = 64 a wave's store is one contiguous KiB). No residual, no weight offsets.
// Every global access of a tensor goes through a range-checked buffer resource with 32-bit offsets.
#include <algorithm>

#include "lds_dma.h"

namespace smpq {
namespace {

constexpr int kS3TH = 8, kS3TW = 16;  // output tile
constexpr int kS3Waves = 4;
constexpr int kS3PF = kS3TH / kS3Waves;  // pixel fragments (tile rows) per wave
constexpr int kS3PW = kS3TW + 2, kS3NPX = (kS3TH + 2) * kS3PW;
constexpr long long kS3BytesMax = 0x7fffff00LL;
static_assert(kS3NPX <= 64 * kS3Waves, "one patch position per thread");

struct Stem3Args {
  const int8_t* xq;       // [3][n][h][w][4]
  long long plane;        // bytes per activation limb plane
  const float* x_absmax;  // [n]
  const int8_t* codes;    // [3][cout][64]
  const float* col_scale;
  const float* col_shift;
  float* y;
  float* y_absmax;
  int8_t* yq;
  int32_t* overflow;
  float yq_inv, inv_qmax;
  int n, h, w, cout, relu;
  int ntw, tiles_img, tiles;
};

// LEAN: the static-range limb-plane epilogue
template <bool LEAN>
__global__ __launch_bounds__(64 * kS3Waves) void qconv_stem3_kernel(Stem3Args a) {
  constexpr int L = 3, LW = 3, NCF = 4;
  constexpr int SMIN = limb_smin(L, LW), NACC = limb_nacc(L, LW);
  __shared__ unsigned patch[2][L][kS3NPX];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int px = lane & 15, grp = lane >> 4;
  const int c0 = blockIdx.x * 64;  // this workgroup's output channels

  // ---- the 64 x 64-byte weight rows of the three limbs, resident for every tile ---------------------
  v4i wreg[LW][NCF];
  {
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(a.codes), 0, LW * a.cout * 64, 0x00020000);
#pragma unroll
    for (int lw = 0; lw < LW; ++lw)
#pragma unroll
      for (int cf = 0; cf < NCF; ++cf)
        wreg[lw][cf] = __builtin_bit_cast(
            v4i, __builtin_amdgcn_raw_buffer_load_b128(
                     wrs, (unsigned)(((lw * a.cout + c0 + 16 * cf + px) * 64) + 16 * grp), 0, 0));
  }
  // dword offsets in a patch limb: of the lane's four taps, and of its pixel in each fragment
  int tapoff[4], pixoff[kS3PF];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tap = 4 * grp + t < 9 ? 4 * grp + t : t;  // K padding (zero codes): group 0's dword
    tapoff[t] = (tap / 3) * kS3PW + tap % 3;
  }
#pragma unroll
  for (int pf = 0; pf < kS3PF; ++pf) pixoff[pf] = (kS3PF * wave + pf) * kS3PW + px;

  const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(a.xq), 0, (int)(L * a.plane), 0x00020000);
  const long long oplane = (long long)a.n * a.h * a.w * a.cout;  // elements per output plane
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y ? (int)(4 * oplane) : 0, 0x00020000);
  const auto qrs = __builtin_amdgcn_make_buffer_rsrc(a.yq, 0, a.yq ? (int)(L * oplane) : 0, 0x00020000);
  constexpr float qmax = act_qmax<L>();
  const bool relu = a.relu != 0;
  const float inv = a.yq_inv;
  float cs[NCF][4], sh[NCF][4];  // LEAN: already in code units (times 1 / output step)
#pragma unroll
  for (int cf = 0; cf < NCF; ++cf) {
    const float4 s = *reinterpret_cast<const float4*>(a.col_scale + c0 + 16 * cf + 4 * grp);
    const float4 b = *reinterpret_cast<const float4*>(a.col_shift + c0 + 16 * cf + 4 * grp);
    cs[cf][0] = s.x, cs[cf][1] = s.y, cs[cf][2] = s.z, cs[cf][3] = s.w;
    sh[cf][0] = b.x, sh[cf][1] = b.y, sh[cf][2] = b.z, sh[cf][3] = b.w;
    if constexpr (LEAN) {
#pragma unroll
      for (int r = 0; r < 4; ++r) cs[cf][r] = cs[cf][r] * inv, sh[cf][r] = sh[cf][r] * inv;
    }
  }
  float vmax = 0.f;  // LEAN: the largest rounded code; otherwise max |y| (both over every tile)

  // the three limb dwords of this thread's patch position of tile t (zero outside the image / the walk)
  unsigned st[L];
  auto fetch = [&](int t) {
    unsigned src = kOOB;
    if (tid < kS3NPX && t < a.tiles) {
      const int img = t / a.tiles_img, rem = t - img * a.tiles_img;
      const int tr = rem / a.ntw, tc = rem - tr * a.ntw;
      const int pr = tid / kS3PW, pc = tid - pr * kS3PW;
      const int ih = tr * kS3TH - 1 + pr, iw = tc * kS3TW - 1 + pc;
      if ((unsigned)ih < (unsigned)a.h && (unsigned)iw < (unsigned)a.w)
        src = (unsigned)(((long long)(img * a.h + ih) * a.w + iw) * 4);
    }
#pragma unroll
    for (int l = 0; l < L; ++l)
      st[l] = __builtin_amdgcn_raw_buffer_load_b32(xrs, src == kOOB ? kOOB : src + (unsigned)(l * a.plane), 0, 0);
  };
  auto stage = [&](int buf) {
    if (tid < kS3NPX) {
#pragma unroll
      for (int l = 0; l < L; ++l) patch[buf][l][tid] = st[l];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  int buf = 0;
  fetch(blockIdx.y);
  stage(0);
  for (int t = blockIdx.y; t < a.tiles; t += gridDim.y, buf ^= 1) {
    fetch(t + gridDim.y);  // in flight over this tile's MFMAs and stores
    const int img = t / a.tiles_img, rem = t - img * a.tiles_img;
    const int tr = rem / a.ntw, tc = rem - tr * a.ntw;
    const int ow = tc * kS3TW + px;
    const float rscale = a.x_absmax[img] * a.inv_qmax;
    float amax = 0.f;
#pragma unroll
    for (int pf = 0; pf < kS3PF; ++pf) {
      // ---- one B fragment per limb, 24 MFMAs --------------------------------------------------------
      v4i fb[L];
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const unsigned* pl = &patch[buf][l][pixoff[pf]];
        fb[l] = v4i{(int)pl[tapoff[0]], (int)pl[tapoff[1]], (int)pl[tapoff[2]], (int)pl[tapoff[3]]};
      }
      v4i acc[NCF][NACC];
#pragma unroll
      for (int cf = 0; cf < NCF; ++cf)
#pragma unroll
        for (int s = 0; s < NACC; ++s) acc[cf][s] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int la = 0; la < L; ++la)
#pragma unroll
        for (int lw = 0; lw < LW; ++lw)
          if (la + lw >= SMIN) {
#pragma unroll
            for (int cf = 0; cf < NCF; ++cf)
              acc[cf][la + lw - SMIN] =
                  __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[lw][cf], fb[la], acc[cf][la + lw - SMIN], 0, 0, 0);
          }

      // ---- epilogue of the fragment: pixel (oh, ow), channels c0 + 16 cf + 4 grp .. + 3 -----------------
      const int oh = tr * kS3TH + kS3PF * wave + pf;
      const bool ok = oh < a.h && ow < a.w;
      const unsigned pix = (unsigned)((img * a.h + oh) * a.w + ow);
      unsigned wq[NCF][L];
#pragma unroll
      for (int cf = 0; cf < NCF; ++cf) {
        if constexpr (LEAN) {
          const int none[4] = {0, 0, 0, 0};
          const float m = lean_quad<L, NACC, SMIN>(acc[cf], rscale, cs[cf], sh[cf], false, none, 0.f, relu,
                                                   relu ? 0.f : -qmax, wq[cf]);
          vmax = ok ? fmaxf(vmax, m) : vmax;
        } else {
          float o[4];
          float am = 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            o[r] = affine(lean_v1<NACC, SMIN>(acc[cf], r), rscale, cs[cf][r], sh[cf][r]);
            if (relu) o[r] = fmaxf(o[r], 0.f);
            am = fmaxf(am, fabsf(o[r]));
          }
          if (ok) amax = fmaxf(amax, am);
          if (a.y) {
            const unsigned eo = pix * (unsigned)a.cout + (unsigned)(c0 + 16 * cf + 4 * grp);
            const v4u v = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])};
            __builtin_amdgcn_raw_buffer_store_b128(v, yrs, ok ? 4u * eo : kOOB, 0, 0);
          }
          if (a.yq) {
            int q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = (int)fminf(fmaxf(rintf(__fmul_rn(o[r], inv)), -qmax), qmax);
            encode4<L>(q, wq[cf]);
          }
        }
      }
      if (a.yq) {
        // lane group g takes the pixel's channels c0 + 16 g .. + 15: one 16-B store per limb
        const unsigned qo = pix * (unsigned)a.cout + (unsigned)(c0 + 16 * grp);
#pragma unroll
        for (int l = 0; l < L; ++l) {
          unsigned w0 = wq[0][l], w1 = wq[1][l], w2 = wq[2][l], w3 = wq[3][l];
          transpose4(w0, w1, w2, w3);
          __builtin_amdgcn_raw_buffer_store_b128(v4u{w0, w1, w2, w3}, qrs, ok ? qo + (unsigned)(l * oplane) : kOOB, 0, 0);
        }
      }
    }
    if constexpr (!LEAN) {
      vmax = fmaxf(vmax, amax);
      if (a.y_absmax) {
        const float m = wave_max(amax);
        if (lane == 0 && m > 0.f) atomic_max_nonneg(&a.y_absmax[img], m);
      }
    }
    stage(buf ^ 1);  // every wave is done with the other stage since the last barrier
  }
  if (a.yq) {
    const bool ovf = LEAN ? vmax > qmax : rintf(__fmul_rn(vmax, a.yq_inv)) > qmax;
    if (__any(ovf) && lane == 0) atomicMax(a.overflow, 1);
  }
}

template <bool LEAN>
int launch_stem3(const Stem3Args& a, hipStream_t stream) {
  const int gx = a.cout / 64;
  // two workgroups per CU in all, what the kernel's ~200 registers keep resident on 256 CUs; each walks
  // tiles from there, so the weights are loaded once per resident workgroup
  int gy = (512 + gx - 1) / gx;
  if (gy > a.tiles) gy = a.tiles;
  hipLaunchKernelGGL(qconv_stem3_kernel<LEAN>, dim3(gx, gy), dim3(64 * kS3Waves), 0, stream, a);
  return check_hip(hipGetLastError(), "qconv_stem3_kernel launch");
}

// NCHW fp32 images (c <= 4 channels) -> 3 int8 limb planes [n][h][w][4], byte ch of a pixel's dword =
// channel ch (zero for ch >= c), quantized with the per-image absmax as act_quantize_kernel does. One
// thread = one pixel: c coalesced loads, one dword store per plane.
__global__ __launch_bounds__(256) void image_quantize_c4_kernel(const float* __restrict__ x, int c, long long hw,
                                                                long long total, const float* __restrict__ absmax,
                                                                unsigned* __restrict__ out) {
  constexpr int L = 3;
  const float qmax = act_qmax<L>();
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (long long)gridDim.x * blockDim.x) {
    const long long img = p / hw, r = p - img * hw;
    const float am = absmax[img];
    const ActScale scale = act_scale<L>(am);
    unsigned word[L] = {0u, 0u, 0u};
    for (int ch = 0; ch < c; ++ch) {
      const float qf = fminf(fmaxf(rintf(scale(x[(img * c + ch) * hw + r])), -qmax), qmax);
      int d[L];
      split_limbs<L>((int)qf, d);
#pragma unroll
      for (int l = 0; l < L; ++l) word[l] |= (unsigned)(d[l] & 255) << (8 * ch);
    }
#pragma unroll
    for (int l = 0; l < L; ++l) out[l * total + p] = word[l];
  }
}

bool stem3_supported(int cin, int cout, int kh, int kw, int stride, int pad, int limbs, int wlimbs) {
  return cin >= 1 && cin <= 4 && cout > 0 && cout % 64 == 0 && kh == 3 && kw == 3 && stride == 1 && pad == 1 &&
         limbs == 3 && wlimbs == 3;
}

}  // namespace
}  // namespace smpq

using namespace smpq;

extern "C" int smpq_stem3_supported(int cin, int cout, int kh, int kw, int stride, int pad, int limbs, int wlimbs) {
  return stem3_supported(cin, cout, kh, kw, stride, pad, limbs, wlimbs) ? 1 : 0;
}

extern "C" int smpq_image_quantize_c4(const float* x, int n, int c, int h, int w, const float* absmax, int8_t* out,
                                      smpq_stream_t stream) {
  if (!x || !absmax || !out || n <= 0 || c <= 0 || c > 4 || h <= 0 || w <= 0)
    return fail(SMPQ_E_INVALID, "smpq_image_quantize_c4: need 1..4 channels and positive sizes");
  if (((uintptr_t)out) & 3) return fail(SMPQ_E_INVALID, "smpq_image_quantize_c4: out must be 4-B aligned");
  const long long hw = (long long)h * w, total = (long long)n * hw;
  const dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 65535));
  hipLaunchKernelGGL(image_quantize_c4_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, c, hw, total, absmax,
                     reinterpret_cast<unsigned*>(out));
  return check_hip(hipGetLastError(), "image_quantize_c4_kernel launch");
}

extern "C" int smpq_stem_conv3_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                 const int8_t* codes, int wlimbs, int cout, int kh, int kw, int stride, int pad,
                                 const float* col_scale, const float* col_shift, int relu, int limbs, float* y,
                                 float* y_absmax, int8_t* yq, float yq_range, int32_t* overflow,
                                 smpq_stream_t stream) {
  if (!xq || !x_absmax || !codes || !col_scale || !col_shift || (!y && !yq))
    return fail(SMPQ_E_INVALID, "smpq_stem_conv3_q: null pointer");
  if (yq && (!overflow || !(yq_range > 0.f)))
    return fail(SMPQ_E_INVALID, "smpq_stem_conv3_q: yq needs overflow flag and a positive range");
  if (n <= 0 || h <= 0 || w <= 0) return fail(SMPQ_E_SHAPE, "smpq_stem_conv3_q: bad shape");
  if (!stem3_supported(cin, cout, kh, kw, stride, pad, limbs, wlimbs))
    return fail(SMPQ_E_SHAPE, "smpq_stem_conv3_q: unsupported geometry (smpq_stem3_supported: 3x3 / stride 1 / pad 1, "
                              "1..4 input channels, cout % 64 == 0, 3 activation and 3 weight limbs)");
  if ((((uintptr_t)xq | (uintptr_t)codes | (uintptr_t)col_scale | (uintptr_t)col_shift | (uintptr_t)y |
        (uintptr_t)yq) & 15) != 0)
    return fail(SMPQ_E_INVALID, "smpq_stem_conv3_q: operands must be 16-B aligned");
  Stem3Args a = {};
  a.plane = (long long)n * h * w * 4;
  const long long oplane = (long long)n * h * w * cout;
  // 32-bit buffer offsets over all three limb planes (and the fp32 output): the caller splits the batch
  if (3 * a.plane > kS3BytesMax || (yq && 3 * oplane > kS3BytesMax) || (y && 4 * oplane > kS3BytesMax) ||
      3LL * cout * 64 > kS3BytesMax)
    return fail(SMPQ_E_SHAPE, "smpq_stem_conv3_q: a tensor of 2 GiB or more (split the batch)");
  a.xq = xq;
  a.x_absmax = x_absmax;
  a.codes = codes;
  a.col_scale = col_scale;
  a.col_shift = col_shift;
  a.y = y;
  a.y_absmax = y_absmax;
  a.yq = yq;
  a.overflow = overflow;
  a.yq_inv = yq ? 8323072.f / yq_range : 0.f;
  a.inv_qmax = 1.f / 8323072.f;
  a.n = n, a.h = h, a.w = w, a.cout = cout, a.relu = relu ? 1 : 0;
  a.ntw = (w + kS3TW - 1) / kS3TW;
  a.tiles_img = ((h + kS3TH - 1) / kS3TH) * a.ntw;
  // (the walk adds gridDim.y <= 512 to a tile index before it compares)
  if ((long long)n * a.tiles_img > 0x7fff0000LL) return fail(SMPQ_E_SHAPE, "smpq_stem_conv3_q: too many tiles");
  a.tiles = n * a.tiles_img;
  const bool lean = yq && !y && !y_absmax;
  return lean ? launch_stem3<true>(a, (hipStream_t)stream) : launch_stem3<false>(a, (hipStream_t)stream);
}
