// Grouped 3x3 quantized conv (pad 1, stride 1 or 2, dilation 1) for gfx950 on
// v_mfma_i32_16x16x64_i8: the conv2 of a ResNeXt Bottleneck (resnet.py:75-78, groups > 1) with its
// eval BatchNorm and ReLU folded in, on 3 activation limbs and 1 or 3 weight limbs.
//
// Block-diagonal fragments. cg = cin / groups, og = cout / groups. The 16 output channels of
// fragment f cover max(1, 16 / og) groups and read the S = cg * max(1, 16 / og) consecutive input
// channels from span(f) = (16 f / og) * cg on. Per fragment K = 9 * S ordered [tap][s], padded with
// zero codes to NK = ceil(9 S / 64) MFMA steps; a code outside its row's own group is zero
// (smpq_weights_grouped_expand). A lane of the MFMA holds 16 consecutive K bytes, i.e. one 16-channel
// chunk of one tap of one pixel: chunk kk = 4 j + (lane >> 4) of step j is tap kk / (S / 16), channels
// 16 (kk % (S / 16)) .. + 15 of the span. Built for S = 16, 32, 64; a span S = cg >= 128 with cg and og
// multiples of 64 goes to the K-streaming kernel of conv_grouped_wide.hip, which reads the same copy.
//
// Weight-stationary. One wave owns one fragment and loads its codes once, NK x 4 VGPRs per weight
// plane, straight from the fragment-ordered copy ([plane][fragment][step][lane][16 B]: one coalesced
// KiB per step). A workgroup is 4 waves = 4 adjacent fragments (64 output channels) and walks 8 x 8
// output tiles: blockIdx.y, + gridDim.y, ... over the n * ceil(ho / 8) * ceil(wo / 8) tiles.
//
// Halo patch in LDS. Per tile the workgroup stages, once and for all nine taps, the 10 x 10 (stride
// 1) or 17 x 17 (stride 2) input pixels of the channels its fragments read, [c_lo, c_lo + cw), for the
// three limb planes, as [limb][pixel][cw] in 1-KiB LDS-DMA pieces (lds_dma.h dma16); a position
// outside the image gets an out-of-range buffer offset, which the DMA stages as zero. A wave's four
// pixel fragments are the tile's row pairs (pixel frow = row 2 pf + frow / 8, column frow % 8), so
// each lane ends with 4 consecutive output channels of 4 pixels. One stage: the next tile's patch is
// issued after every wave has read the last one.
//
// Weight offsets (one weight limb: weight = code + offset[c]). The correction is offset[c] times the
// window sum of the digits of the row's OWN group. The expanded copy carries one more plane, the
// group indicator (1 inside the row's group, 0 elsewhere and in the K padding): one MFMA of it per
// activation limb yields those sums from the staged patch in the accumulator layout, whatever og is.
//
// Epilogue: conv_common.h / lds_dma.h arithmetic (limb_smin / limb_nacc passes, lean_v1, affine,
// lean_quad, encode4), so a value is rounded as the dense kernels round it: the lean static-range
// form when only limb planes are wanted, the general form (fp32 y, y_absmax, limb planes) otherwise.
// Every global access of a tensor goes through a range-checked buffer resource with 32-bit offsets.
#include "lds_dma.h"

namespace smpq {
namespace {

constexpr int kGT = 8;                // output tile edge
constexpr int kGWaves = 4;            // fragments per workgroup
constexpr int kGLdsMax = 160 * 1024;  // LDS per workgroup on gfx950
constexpr long long kGBytesMax = 0x7fffff00LL;

__host__ __device__ inline int grouped_span(int f, int cg, int og) { return (16 * f / og) * cg; }
inline int grouped_S(int cg, int og) { return cg * (og >= 16 ? 1 : 16 / og); }
__host__ __device__ constexpr int grouped_nk(int spf) { return (9 * spf + 3) / 4; }
__host__ __device__ constexpr int grouped_patch(int stride) { return stride * (kGT - 1) + 3; }

// channels a workgroup stages: from its first fragment's span to the end of its last one's
__host__ __device__ inline void grouped_block_span(int cb, int nfrag, int cg, int og, int S, int& c_lo, int& cw) {
  const int f0 = cb * kGWaves, f1 = (f0 + kGWaves < nfrag ? f0 + kGWaves : nfrag) - 1;
  c_lo = grouped_span(f0, cg, og);
  cw = grouped_span(f1, cg, og) + S - c_lo;
}

inline int grouped_lds_bytes(int nfrag, int cg, int og, int S, int stride) {
  int cwmax = 0;
  for (int cb = 0; cb * kGWaves < nfrag; ++cb) {
    int c_lo, cw;
    grouped_block_span(cb, nfrag, cg, og, S, c_lo, cw);
    cwmax = cw > cwmax ? cw : cwmax;
  }
  const int px = grouped_patch(stride) * grouped_patch(stride);
  return (3 * px * cwmax + 1023) / 1024 * 1024;  // whole DMA pieces
}

// LW weight limbs (1 or 3), OFF: weight offsets (LW == 1), SPF = S / 16, STRIDE 1 or 2, LEAN: the
// static-range limb-plane epilogue
template <int LW, bool OFF, int SPF, int STRIDE, bool LEAN>
__global__ __launch_bounds__(64 * kGWaves) void qconv_grouped_kernel(GroupedArgs a) {
  constexpr int L = 3;
  constexpr int SMIN = limb_smin(L, LW), NACC = limb_nacc(L, LW);
  constexpr int NK = grouped_nk(SPF);
  constexpr int PW = grouped_patch(STRIDE), NPX = PW * PW;
  constexpr int WP = LW + (OFF ? 1 : 0);  // weight planes held (the last one: the group indicator)
  constexpr int NPF = kGT * kGT / 16;     // pixel fragments of a tile
  static_assert(NPF == 4, "the limb-plane stores transpose four pixel fragments");
  extern __shared__ __attribute__((aligned(1024))) int8_t lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int frow = lane & 15, grp = lane >> 4;
  const int f = blockIdx.x * kGWaves + wave;
  const bool active = f < a.nfrag;
  int c_lo, cw;
  grouped_block_span(blockIdx.x, a.nfrag, a.cg, a.og, 16 * SPF, c_lo, cw);
  const int cwc = cw / 16;           // 16-B chunks per staged pixel
  const int plimb = NPX * cw;        // LDS bytes per limb
  const int chunks = L * NPX * cwc;  // 16-B chunks of the patch image
  const int pieces = (chunks + 63) / 64;

  // ---- this wave's fragment, resident in registers for every tile ------------------------------
  v4i wreg[WP][NK];
  {
    const long long wplane = (long long)a.nfrag * NK * 1024;
    const int fr = active ? f : 0;
#pragma unroll
    for (int p = 0; p < WP; ++p)
#pragma unroll
      for (int j = 0; j < NK; ++j)
        wreg[p][j] = *reinterpret_cast<const v4i*>(a.wexp + p * wplane + ((long long)fr * NK + j) * 1024 + lane * 16);
  }
  // per-lane LDS offsets: of the lane's tap chunk in each K step, and of its pixel in each fragment
  int tapoff[NK], pixoff[NPF];
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int kk = 4 * j + grp, tap = kk / SPF, sub = kk - tap * SPF;
    tapoff[j] = tap < 9 ? ((tap / 3) * PW + tap % 3) * cw + 16 * sub : 0;  // K padding: the codes are zero
  }
  const int fragoff = active ? grouped_span(f, a.cg, a.og) - c_lo : 0;
#pragma unroll
  for (int pf = 0; pf < NPF; ++pf)
    pixoff[pf] = (STRIDE * (2 * pf + (frow >> 3)) * PW + STRIDE * (frow & 7)) * cw + fragoff;

  const v4i xrs = make_rsrc(a.xq, (long long)L * a.plane);
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds));
  const long long oplane = (long long)a.n * a.ho * a.wo * a.cout;  // elements per output plane
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y ? (int)(4 * oplane) : 0, 0x00020000);
  const auto qrs = __builtin_amdgcn_make_buffer_rsrc(a.yq, 0, a.yq ? (int)(L * oplane) : 0, 0x00020000);
  const int c4 = 16 * (active ? f : 0) + 4 * grp;  // this lane's 4 output channels
  const float4 cs = *reinterpret_cast<const float4*>(a.col_scale + c4);
  const float4 csh = *reinterpret_cast<const float4*>(a.col_shift + c4);
  int cor[4] = {0, 0, 0, 0};
  if constexpr (OFF) {
    const int4 o = *reinterpret_cast<const int4*>(a.w_off + c4);
    cor[0] = o.x, cor[1] = o.y, cor[2] = o.z, cor[3] = o.w;
  }
  constexpr float qmax = act_qmax<L>();
  const bool relu = a.relu != 0;
  float vmax = 0.f;  // LEAN: the largest rounded code; otherwise max |y| (both over every tile)

  for (int t = blockIdx.y; t < a.tiles; t += gridDim.y) {
    const int img = t / a.tiles_img, rem = t - img * a.tiles_img;
    const int tr = rem / a.ntw, tc = rem - tr * a.ntw;
    const int oh0 = tr * kGT, ow0 = tc * kGT;
    const int ih0 = oh0 * STRIDE - 1, iw0 = ow0 * STRIDE - 1;
    if (t != (int)blockIdx.y) {  // every wave is done with the last patch
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    // ---- stage the patch: piece p = LDS bytes [1024 p, + 1024), lane i its chunk 64 p + i ---------
    for (int p = wave; p < pieces; p += kGWaves) {
      const int q = 64 * p + lane;
      unsigned src = kOOB;
      if (q < chunks) {
        const int l = q / (NPX * cwc), r1 = q - l * (NPX * cwc);
        const int px = r1 / cwc, ch = r1 - px * cwc;
        const int pr = px / PW, pc = px - pr * PW;
        const int ih = ih0 + pr, iw = iw0 + pc;
        if ((unsigned)ih < (unsigned)a.h && (unsigned)iw < (unsigned)a.w)
          src = (unsigned)(l * a.plane + ((long long)(img * a.h + ih) * a.w + iw) * a.cin + c_lo + 16 * ch);
      }
      dma16(__builtin_amdgcn_readfirstlane(lds0 + (unsigned)p * 1024u), xrs, src, 0u);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (!active) continue;  // (wave-uniform; the barriers above are reached by every wave)

    // ---- all nine taps out of LDS ------------------------------------------------------------------
    v4i acc[NACC][NPF], gs[OFF ? L : 1][NPF];
#pragma unroll
    for (int pf = 0; pf < NPF; ++pf) {
#pragma unroll
      for (int s = 0; s < NACC; ++s) acc[s][pf] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int l = 0; l < (OFF ? L : 1); ++l) gs[l][pf] = v4i{0, 0, 0, 0};
    }
#pragma unroll
    for (int j = 0; j < NK; ++j)
#pragma unroll
      for (int pf = 0; pf < NPF; ++pf) {
        v4i fb[L];
#pragma unroll
        for (int l = 0; l < L; ++l) fb[l] = *reinterpret_cast<const v4i*>(lds + l * plimb + pixoff[pf] + tapoff[j]);
#pragma unroll
        for (int la = 0; la < L; ++la) {
#pragma unroll
          for (int lw = 0; lw < LW; ++lw)
            if (la + lw >= SMIN)
              acc[la + lw - SMIN][pf] =
                  __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[lw][j], fb[la], acc[la + lw - SMIN][pf], 0, 0, 0);
          if constexpr (OFF)
            gs[la][pf] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[LW][j], fb[la], gs[la][pf], 0, 0, 0);
        }
      }
    if constexpr (OFF) {  // weight = code + offset: + offset[c] * (window sum of the group's digits)
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int pf = 0; pf < NPF; ++pf)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[l][pf][r] += cor[r] * gs[l][pf][r];
    }

    // ---- epilogue ---------------------------------------------------------------------------------
    const float rscale = a.x_absmax[img] * a.inv_qmax;
    const float inv = a.yq_inv;
    unsigned wq[NPF][L];
    float amax = 0.f;
#pragma unroll
    for (int pf = 0; pf < NPF; ++pf) {
      const int oh = oh0 + 2 * pf + (frow >> 3), ow = ow0 + (frow & 7);
      const bool ok = oh < a.ho && ow < a.wo;
      v4i accq[NACC];
#pragma unroll
      for (int s = 0; s < NACC; ++s) accq[s] = acc[s][pf];
      if constexpr (LEAN) {
        const float csq[4] = {cs.x * inv, cs.y * inv, cs.z * inv, cs.w * inv};
        const float shq[4] = {csh.x * inv, csh.y * inv, csh.z * inv, csh.w * inv};
        const int none[4] = {0, 0, 0, 0};
        const float m = lean_quad<L, NACC, SMIN>(accq, rscale, csq, shq, false, none, 0.f, relu, relu ? 0.f : -qmax,
                                                 wq[pf]);
        vmax = ok ? fmaxf(vmax, m) : vmax;
      } else {
        const float csr[4] = {cs.x, cs.y, cs.z, cs.w}, shr[4] = {csh.x, csh.y, csh.z, csh.w};
        float o[4];
        float am = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[r] = affine(lean_v1<NACC, SMIN>(accq, r), rscale, csr[r], shr[r]);
          if (relu) o[r] = fmaxf(o[r], 0.f);
          am = fmaxf(am, fabsf(o[r]));
        }
        if (ok) amax = fmaxf(amax, am);
        if (a.y) {
          const unsigned eo = (unsigned)(((long long)(img * a.ho + oh) * a.wo + ow) * a.cout + c4);
          const v4u v = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])};
          __builtin_amdgcn_raw_buffer_store_b128(v, yrs, ok ? 4u * eo : kOOB, 0, 0);
        }
        if (a.yq) {
          int q[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) q[r] = (int)fminf(fmaxf(rintf(__fmul_rn(o[r], inv)), -qmax), qmax);
          encode4<L>(q, wq[pf]);
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
    if (a.yq) {
      // lane group g takes pixel fragment g: the 16 channels of the fragment, one 16-B store per limb
      const int oh = oh0 + 2 * grp + (frow >> 3), ow = ow0 + (frow & 7);
      const bool ok = oh < a.ho && ow < a.wo;
      const unsigned qo = (unsigned)(((long long)(img * a.ho + oh) * a.wo + ow) * a.cout + 16 * f);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        unsigned w0 = wq[0][l], w1 = wq[1][l], w2 = wq[2][l], w3 = wq[3][l];
        transpose4(w0, w1, w2, w3);
        __builtin_amdgcn_raw_buffer_store_b128(v4u{w0, w1, w2, w3}, qrs, ok ? qo + (unsigned)(l * oplane) : kOOB, 0, 0);
      }
    }
  }
  if (a.yq && active) {
    const bool ovf = LEAN ? vmax > qmax : rintf(__fmul_rn(vmax, a.yq_inv)) > qmax;
    if (__any(ovf) && lane == 0) atomicMax(a.overflow, 1);
  }
}

template <int LW, bool OFF, int SPF, int STRIDE, bool LEAN>
int launch_grouped_one(const GroupedArgs& a, int lds_bytes, hipStream_t stream) {
  const auto fn = qconv_grouped_kernel<LW, OFF, SPF, STRIDE, LEAN>;
  static const hipError_t attr = [&] {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kGLdsMax);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  }();
  if (attr != hipSuccess) return check_hip(attr, "qconv_grouped_kernel LDS attribute");
  const int gx = (a.nfrag + kGWaves - 1) / kGWaves;
  int gy = (1024 + gx - 1) / gx;  // about four workgroups per CU in all; each walks tiles from there
  if (gy > a.tiles) gy = a.tiles;
  hipLaunchKernelGGL(fn, dim3(gx, gy), dim3(64 * kGWaves), lds_bytes, stream, a);
  return check_hip(hipGetLastError(), "qconv_grouped_kernel launch");
}

template <int LW, bool OFF, int SPF>
int launch_grouped_s(const GroupedArgs& a, int stride, bool lean, int lds_bytes, hipStream_t s) {
  if (stride == 1)
    return lean ? launch_grouped_one<LW, OFF, SPF, 1, true>(a, lds_bytes, s)
                : launch_grouped_one<LW, OFF, SPF, 1, false>(a, lds_bytes, s);
  return lean ? launch_grouped_one<LW, OFF, SPF, 2, true>(a, lds_bytes, s)
              : launch_grouped_one<LW, OFF, SPF, 2, false>(a, lds_bytes, s);
}

template <int LW, bool OFF>
int launch_grouped_w(const GroupedArgs& a, int spf, int stride, bool lean, int lds_bytes, hipStream_t s) {
  switch (spf) {
    case 1: return launch_grouped_s<LW, OFF, 1>(a, stride, lean, lds_bytes, s);
    case 2: return launch_grouped_s<LW, OFF, 2>(a, stride, lean, lds_bytes, s);
    default: return launch_grouped_s<LW, OFF, 4>(a, stride, lean, lds_bytes, s);
  }
}

// compact codes [wlimbs][cout][9 cg] -> [planes][nfrag][nk][64 lanes][16 B], one byte per thread
__global__ void grouped_expand_kernel(const int8_t* __restrict__ codes, int wlimbs, int cout, int cg, int og, int S,
                                      int nk, int nfrag, int8_t* __restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i & 15), lane = (int)((i >> 4) & 63);
  long long rest = i >> 10;
  const int j = (int)(rest % nk);
  rest /= nk;
  const int f = (int)(rest % nfrag), p = (int)(rest / nfrag);
  const int row = 16 * f + (lane & 15), k = 64 * j + 16 * (lane >> 4) + b;
  const int tap = k / S, s = k - tap * S;
  int v = 0;
  if (tap < 9) {
    const int ch = grouped_span(f, cg, og) + s, g = row / og;
    if (ch / cg == g) v = p < wlimbs ? codes[((long long)p * cout + row) * (9 * cg) + tap * cg + (ch - g * cg)] : 1;
  }
  out[i] = (int8_t)v;
}

long long grouped_expand_bytes(int wlimbs, int cout, int cg, int og) {
  return (long long)(wlimbs + (wlimbs == 1 ? 1 : 0)) * (cout / 16) * grouped_nk(grouped_S(cg, og) / 16) * 1024;
}

bool grouped_supported(int cin, int cout, int groups, int kh, int kw, int stride, int pad, int limbs, int wlimbs) {
  if (groups < 2 || cin <= 0 || cout <= 0 || cin % groups != 0 || cout % groups != 0) return false;
  if (kh != 3 || kw != 3 || pad != 1 || (stride != 1 && stride != 2)) return false;
  if (limbs != 3 || (wlimbs != 1 && wlimbs != 3)) return false;
  if (cin % 16 != 0 || cout % 16 != 0) return false;
  const int cg = cin / groups, og = cout / groups;
  if (!(og <= 16 ? 16 % og == 0 : og % 16 == 0)) return false;
  const int S = grouped_S(cg, og);
  // conv_grouped_wide.hip: whole 64-channel K chunks, a workgroup's 64 channels inside one group; the
  // expanded copy within its 32-bit buffer offsets
  if (grouped_wide_shape(cg, og)) return grouped_expand_bytes(wlimbs, cout, cg, og) <= kGBytesMax;
  if (S != 16 && S != 32 && S != 64) return false;
  return grouped_lds_bytes(cout / 16, cg, og, S, stride) <= kGLdsMax;
}

}  // namespace
}  // namespace smpq

using namespace smpq;

extern "C" int smpq_conv2d_grouped_supported(int cin, int cout, int groups, int kh, int kw, int stride, int pad,
                                             int limbs, int wlimbs) {
  return grouped_supported(cin, cout, groups, kh, kw, stride, pad, limbs, wlimbs) ? 1 : 0;
}

extern "C" size_t smpq_weights_grouped_expand_bytes(int wlimbs, int cout, int cg, int groups) {
  if (groups < 2 || cout <= 0 || cg <= 0 || cout % groups != 0 ||
      !grouped_supported(cg * groups, cout, groups, 3, 3, 1, 1, 3, wlimbs))
    return 0;
  return (size_t)grouped_expand_bytes(wlimbs, cout, cg, cout / groups);
}

extern "C" int smpq_weights_grouped_expand(const int8_t* codes, int wlimbs, int cout, int cg, int groups, int8_t* out,
                                           smpq_stream_t stream) {
  if (!codes || !out) return fail(SMPQ_E_INVALID, "smpq_weights_grouped_expand: null pointer");
  if (((uintptr_t)out) & 15) return fail(SMPQ_E_INVALID, "smpq_weights_grouped_expand: out must be 16-B aligned");
  if (smpq_weights_grouped_expand_bytes(wlimbs, cout, cg, groups) == 0)
    return fail(SMPQ_E_SHAPE, "smpq_weights_grouped_expand: not a grouped 3x3 operand the kernel takes "
                              "(smpq_conv2d_grouped_supported)");
  const int og = cout / groups, S = grouped_S(cg, og), nk = grouped_nk(S / 16), nfrag = cout / 16;
  const long long total = grouped_expand_bytes(wlimbs, cout, cg, og);
  hipLaunchKernelGGL(grouped_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     codes, wlimbs, cout, cg, og, S, nk, nfrag, out, total);
  return check_hip(hipGetLastError(), "grouped_expand_kernel launch");
}

extern "C" int smpq_conv2d_grouped_fwd_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                         const int8_t* codes, const int8_t* codes_expanded, int wlimbs,
                                         const int32_t* offset, int cout, int groups, int kh, int kw, int stride,
                                         int pad, const float* col_scale, const float* col_shift, int relu, int limbs,
                                         float* y, float* y_absmax, int8_t* yq, float yq_range, int32_t* overflow,
                                         smpq_stream_t stream) {
  if (!xq || !x_absmax || !codes || !codes_expanded || !col_scale || !col_shift || (!y && !yq))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_grouped_fwd_q: null pointer");
  if (yq && (!overflow || !(yq_range > 0.f)))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_grouped_fwd_q: yq needs overflow flag and a positive range");
  if (limbs != 3 || (wlimbs != 1 && wlimbs != 3))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_grouped_fwd_q: built for 3 activation limbs and 1 or 3 weight limbs");
  if (n <= 0 || h <= 0 || w <= 0) return fail(SMPQ_E_SHAPE, "smpq_conv2d_grouped_fwd_q: bad shape");
  if (!grouped_supported(cin, cout, groups, kh, kw, stride, pad, limbs, wlimbs))
    return fail(SMPQ_E_SHAPE, "smpq_conv2d_grouped_fwd_q: unsupported geometry (smpq_conv2d_grouped_supported: 3x3 / "
                              "pad 1 / stride 1 or 2, groups >= 2, cin % 16 == 0, cout % 16 == 0, cout / groups "
                              "dividing or divided by 16, a fragment span of 16, 32 or 64 channels, or cin / groups "
                              ">= 128 with cin / groups and cout / groups multiples of 64)");
  if ((((uintptr_t)xq | (uintptr_t)codes_expanded | (uintptr_t)col_scale | (uintptr_t)col_shift | (uintptr_t)offset |
        (uintptr_t)y | (uintptr_t)yq) & 15) != 0)
    return fail(SMPQ_E_INVALID, "smpq_conv2d_grouped_fwd_q: operands must be 16-B aligned");
  GroupedArgs a = {};
  a.ho = (h + 2 - 3) / stride + 1;
  a.wo = (w + 2 - 3) / stride + 1;
  a.plane = (long long)n * h * w * cin;
  const long long oplane = (long long)n * a.ho * a.wo * cout;
  // 32-bit buffer offsets over all three limb planes (and the fp32 output): the caller splits the batch
  if (3 * a.plane > kGBytesMax || (yq && 3 * oplane > kGBytesMax) || (y && 4 * oplane > kGBytesMax))
    return fail(SMPQ_E_SHAPE, "smpq_conv2d_grouped_fwd_q: a tensor of 2 GiB or more (split the batch)");
  a.xq = xq;
  a.x_absmax = x_absmax;
  a.wexp = codes_expanded;
  a.w_off = wlimbs == 1 ? offset : nullptr;
  a.col_scale = col_scale;
  a.col_shift = col_shift;
  a.y = y;
  a.y_absmax = y_absmax;
  a.yq = yq;
  a.overflow = overflow;
  a.yq_inv = yq ? 8323072.f / yq_range : 0.f;
  a.inv_qmax = 1.f / 8323072.f;
  a.n = n, a.h = h, a.w = w, a.cin = cin, a.cout = cout;
  a.cg = cin / groups, a.og = cout / groups, a.nfrag = cout / 16, a.relu = relu ? 1 : 0;
  a.ntw = (a.wo + kGT - 1) / kGT;
  a.tiles_img = ((a.ho + kGT - 1) / kGT) * a.ntw;
  if ((long long)n * a.tiles_img > 0x7fffffffLL) return fail(SMPQ_E_SHAPE, "smpq_conv2d_grouped_fwd_q: too many tiles");
  a.tiles = n * a.tiles_img;
  const bool lean = yq && !y && !y_absmax;
  hipStream_t s = (hipStream_t)stream;
  if (grouped_wide_shape(a.cg, a.og)) return launch_grouped_wide(a, wlimbs, stride, lean, s);
  const int S = grouped_S(a.cg, a.og);
  const int lds_bytes = grouped_lds_bytes(a.nfrag, a.cg, a.og, S, stride);
  if (wlimbs == 3) return launch_grouped_w<3, false>(a, S / 16, stride, lean, lds_bytes, s);
  return a.w_off ? launch_grouped_w<1, true>(a, S / 16, stride, lean, lds_bytes, s)
                 : launch_grouped_w<1, false>(a, S / 16, stride, lean, lds_bytes, s);
}
