// Wide-group 3x3 quantized conv (pad 1, stride 1 or 2, dilation 1) for gfx950 on
// v_mfma_i32_16x16x64_i8: the conv2 of a ResNeXt Bottleneck whose groups are wide (32x16d, 32x32d, any
// low group count), eval BatchNorm and ReLU folded in, on 3 activation limbs and 1 or 3 weight limbs.
//
// Rule. cg = cin / groups and og = cout / groups are multiples of 64 and cg >= 128 (cg = 64 stays with
// conv_grouped.hip, whose fragment holds its whole K in registers). A fragment of 16 output channels
// then reads exactly its own group's cg channels: K = 9 cg ordered [tap][s], 9 cg / 64 whole MFMA
// steps, no zero padding and no foreign group inside a fragment. The weights are the fragment-ordered
// copy of smpq_weights_grouped_expand, [plane][fragment][step][lane][16 B], unchanged.
//
// Work split. A workgroup is 4 waves and owns 64 consecutive output channels, which lie inside one
// group g because og % 64 == 0; it walks 8 x 8 output tiles blockIdx.y, + gridDim.y, ... over the
// n * ceil(ho / 8) * ceil(wo / 8) tiles. Wave v owns fragment 4 blockIdx.x + v against the tile's four
// pixel fragments (pixel frow of fragment pf = tile row 2 pf + frow / 8, column frow % 8), so a lane
// ends with 4 consecutive output channels of 4 pixels. Accumulators follow limb_smin / limb_nacc.
//
// K is streamed in 64-channel chunks kc of the group: channels g cg + 64 kc .. + 63 of an NHWC pixel.
//
// Activations. Per chunk the workgroup stages the halo patch (10 x 10 at stride 1, 17 x 17 at stride
// 2) of the three limb planes by LDS-DMA (lds_dma.h dma16) in 1-KiB pieces, wave v the pieces v, v + 4,
// ...; a position outside the image gets the out-of-range buffer offset, which the DMA stages as zero.
// All nine taps of the chunk read that patch. A lane's sources depend on the tile only; the chunk moves
// the scalar offset.
//   * Stride 1: two stages of 19 KiB. While the MFMAs of chunk q run, the pieces of chunk q + 1 (the
//     next tile's first chunk after a tile's last one) are issued a few per tap into the other stage,
//     so one barrier per chunk serves both "landed" and "free to overwrite".
//   * Stride 2: one stage of 55 KiB, refilled between two barriers per chunk. Two stages (110 KiB)
//     would leave one workgroup = one wave per SIMD on a CU, with nothing to run under a wave's LDS
//     reads or its epilogue; one stage keeps two workgroups on a CU, and each runs under the other's
//     refill.
//
// LDS image and its conflict count. [limb][ri][ci][64 B]: patch row pr sits at image row ri = pr
// (stride 1) or ri = 9 (pr & 1) + (pr >> 1) (stride 2: even rows first, then odd ones; columns
// likewise), and the 16-B chunk c of a pixel at c ^ 2 (ri & 1). The pixels of a fragment read, patch
// (STRIDE r + kr, STRIDE c + kc), are then image pixels (r + const, c + const) at both strides: two
// runs of 8 adjacent pixels, one image row apart. Enumerating every tap, pixel fragment and
// ds_read_b128 lane group of gfx950 as tools/halo_conflicts.py does gives 0 extra LDS cycles at both
// strides (tools/grouped_wide_conflicts.py; the stride-1 image is conv_halo.hip's; at stride 2 the
// plain row-major 17 x 17 image costs 3 extra cycles on every read and no XOR of the chunk index
// brings it below 1, because patch pixels two apart fall on only two of the four 64-B bank quarters).
// The DMA writes LDS lane-linearly, so the permutation is applied to its per-lane sources.
//
// Weights go straight to registers: for chunk kc, tap t is step t (cg / 64) + kc of the fragment, one
// coalesced KiB per weight plane, loaded two taps ahead of use into a ring of three taps (3 LW x 4
// VGPRs; taps 7 and 8 fetch taps 0 and 1 of the next chunk), never a whole chunk's nine steps.
//
// Weight offsets (one weight limb: weight = code + offset[c]). Every staged channel belongs to the
// row's own group, so the correction is offset[c] times the digit sum of the staged window, taken with
// v_dot4 on the B fragments; the indicator plane of the expanded copy is not read.
//
// Epilogue: conv_common.h / lds_dma.h arithmetic (lean_v1, affine, lean_quad, encode4, transpose4), so
// a value is rounded as the other kernels round it: the lean static-range form when only limb planes
// are wanted, the general form (fp32 y, y_absmax, limb planes) otherwise. No residual. Every global
// access (activations, weights, outputs) goes through a range-checked buffer resource with 32-bit
// offsets.
#include "lds_dma.h"

namespace smpq {
namespace {

constexpr int kWT = 8;      // output tile edge
constexpr int kWWaves = 4;  // fragments per workgroup

__host__ __device__ constexpr int wide_patch(int stride) { return stride * (kWT - 1) + 3; }
// 1-KiB DMA pieces of one stage: [3 limbs][patch pixels][64 B]
__host__ __device__ constexpr int wide_pieces(int stride) {
  return (3 * wide_patch(stride) * wide_patch(stride) * 64 + 1023) / 1024;
}
__host__ __device__ constexpr int wide_stages(int stride) { return stride == 1 ? 2 : 1; }
// image row / column of patch row / column p, and its inverse
template <int STRIDE>
__device__ constexpr int wide_idx(int p) {
  return STRIDE == 1 ? p : 9 * (p & 1) + (p >> 1);
}
template <int STRIDE>
__device__ __forceinline__ int wide_pos(int i) {
  return STRIDE == 1 ? i : (i < 9 ? 2 * i : 2 * (i - 9) + 1);
}

// LW weight limbs (1 or 3), OFF: weight offsets (LW == 1), STRIDE 1 or 2, LEAN: the static-range
// limb-plane epilogue
template <int LW, bool OFF, int STRIDE, bool LEAN>
__global__ __launch_bounds__(64 * kWWaves, 2) void qconv_grouped_wide_kernel(GroupedArgs a) {
  constexpr int L = 3;
  constexpr int SMIN = limb_smin(L, LW), NACC = limb_nacc(L, LW);
  constexpr int PW = wide_patch(STRIDE), NPX = PW * PW, PLIMB = NPX * 64;
  constexpr int PIECES = wide_pieces(STRIDE), STAGE = PIECES * 1024, NST = wide_stages(STRIDE);
  constexpr int PSL = (PIECES + kWWaves - 1) / kWWaves;  // pieces a wave stages per chunk
  constexpr int PPT = (PSL + 8) / 9;                     // of them issued per tap (two stages)
  constexpr int NPF = kWT * kWT / 16;                    // pixel fragments of a tile
  static_assert(NPF == 4, "the limb-plane stores transpose four pixel fragments");
  static_assert(!OFF || LW == 1, "weight offsets come with one weight limb");
  extern __shared__ __attribute__((aligned(1024))) int8_t lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __builtin_assume(wave >= 0 && wave < kWWaves);
  const int frow = lane & 15, grp = lane >> 4;
  const int f = blockIdx.x * kWWaves + wave;  // (nfrag % 4 == 0: every wave has a fragment)
  const int nch = a.cg / 64, nk = 9 * nch;
  const unsigned cbase = (unsigned)((int)(blockIdx.x * 64) / a.og * a.cg);  // the group's first input channel

  const v4i xrs = make_rsrc(a.xq, (long long)L * a.plane);
  const unsigned wplane = (unsigned)a.nfrag * (unsigned)nk * 1024u;
  const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(a.wexp), 0, (int)((LW == 1 ? 2u : 3u) * wplane),
                                                     0x00020000);
  const unsigned wvoff = (unsigned)f * (unsigned)nk * 1024u + 16u * (unsigned)lane;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds));
  const long long oplane = (long long)a.n * a.ho * a.wo * a.cout;  // elements per output plane
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y ? (int)(4 * oplane) : 0, 0x00020000);
  const auto qrs = __builtin_amdgcn_make_buffer_rsrc(a.yq, 0, a.yq ? (int)(L * oplane) : 0, 0x00020000);
  const int c4 = 16 * f + 4 * grp;  // this lane's 4 output channels
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

  // ---- staging: the per-lane sources of tile t, and the issue of piece wave + 4 k ------------------
  unsigned psrc[PSL];
  auto tile_src = [&](int t) {
    const int img = t / a.tiles_img, rem = t - img * a.tiles_img;
    const int tr = rem / a.ntw, tc = rem - tr * a.ntw;
    const int ih0 = tr * kWT * STRIDE - 1, iw0 = tc * kWT * STRIDE - 1;
#pragma unroll
    for (int k = 0; k < PSL; ++k) {
      const int q = 64 * (wave + kWWaves * k) + lane;  // 16-B position of the stage image
      const int l = q / (4 * NPX), r1 = q - l * (4 * NPX);
      const int pix = r1 >> 2, ri = pix / PW, ci = pix - ri * PW;
      const int ih = ih0 + wide_pos<STRIDE>(ri), iw = iw0 + wide_pos<STRIDE>(ci);
      const int ch = (r1 & 3) ^ (2 * (ri & 1));
      const bool ok = l < L && (unsigned)ih < (unsigned)a.h && (unsigned)iw < (unsigned)a.w;
      psrc[k] = ok ? (unsigned)(l * a.plane + ((long long)(img * a.h + ih) * a.w + iw) * a.cin + 16 * ch) : kOOB;
    }
  };
  auto issue = [&](int k, unsigned stage, unsigned soff) {
    if (wave + kWWaves * k < PIECES)
      dma16(__builtin_amdgcn_readfirstlane(lds0 + stage + (unsigned)(wave + kWWaves * k) * 1024u), xrs, psrc[k], soff);
  };
  // ---- weights: the LW planes of one K step of this wave's fragment --------------------------------
  v4i wreg[3][LW];
  auto wload = [&](int step, v4i* dst) {
#pragma unroll
    for (int lw = 0; lw < LW; ++lw)
      dst[lw] = (v4i)__builtin_amdgcn_raw_buffer_load_b128(
          wrs, wvoff, __builtin_amdgcn_readfirstlane((unsigned)lw * wplane + (unsigned)step * 1024u), 0);
  };
  // per-lane fragment bases: this lane's pixel of fragment 0, for an even ([0]) and an odd ([1]) image row
  // offset of the tap (the row parity flips the chunk XOR)
  int bpar[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    bpar[par] = ((frow >> 3) * PW + (frow & 7)) * 64 + 16 * (grp ^ (2 * (((frow >> 3) + par) & 1)));

  int t = blockIdx.y;
  unsigned seq = 0;  // chunks done: the ring's stage is seq & 1
  tile_src(t);
#pragma unroll
  for (int k = 0; k < PSL; ++k) issue(k, 0u, __builtin_amdgcn_readfirstlane(cbase));
  wload(0, wreg[0]);
  wload(nch, wreg[1]);

  for (; t < a.tiles; t += gridDim.y) {
    const int img = t / a.tiles_img, rem = t - img * a.tiles_img;
    const int tr = rem / a.ntw, tc = rem - tr * a.ntw;
    const int oh0 = tr * kWT, ow0 = tc * kWT;
    v4i acc[NACC][NPF];
    int rs[L][NPF];  // OFF: this lane's share of the window digit sums
#pragma unroll
    for (int pf = 0; pf < NPF; ++pf) {
#pragma unroll
      for (int s = 0; s < NACC; ++s) acc[s][pf] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int l = 0; l < L; ++l) rs[l][pf] = 0;
    }

    for (int kc = 0; kc < nch; ++kc, ++seq) {
      // what is staged next: this tile's next chunk, or the first chunk of the workgroup's next tile
      const bool last = kc + 1 == nch;
      const int tn = last ? t + (int)gridDim.y : t, kn = last ? 0 : kc + 1;
      const bool more = tn < a.tiles;
      const unsigned soffn = __builtin_amdgcn_readfirstlane(cbase + 64u * (unsigned)kn);
      const unsigned stc = NST == 2 ? (seq & 1u) * STAGE : 0u, stn = NST == 2 ? STAGE - stc : 0u;
      if (NST == 2 && last && more) tile_src(tn);  // (this tile's last chunk was issued a chunk ago)
      // chunk seq has landed, and every wave is done reading chunk seq - 1
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        if (NST == 2 && more) {
#pragma unroll
          for (int k = tap * PPT; k < (tap + 1) * PPT && k < PSL; ++k) issue(k, stn, soffn);
        }
        wload(tap + 2 < 9 ? (tap + 2) * nch + kc : (tap + 2 - 9) * nch + kn, wreg[(tap + 2) % 3]);
        const int kr = tap / 3, kcol = tap % 3;
        const int ro = wide_idx<STRIDE>(kr), co = wide_idx<STRIDE>(kcol);  // the tap's image offset
        const int8_t* base = lds + stc + bpar[ro & 1] + (ro * PW + co) * 64;
#pragma unroll
        for (int pf = 0; pf < NPF; ++pf) {
          v4i fb[L];
#pragma unroll
          for (int l = 0; l < L; ++l) fb[l] = *reinterpret_cast<const v4i*>(base + l * PLIMB + pf * (2 * PW * 64));
          if constexpr (OFF) {
#pragma unroll
            for (int l = 0; l < L; ++l) {
              int sacc = rs[l][pf];
              sacc = __builtin_amdgcn_sdot4(fb[l].x, 0x01010101, sacc, false);
              sacc = __builtin_amdgcn_sdot4(fb[l].y, 0x01010101, sacc, false);
              sacc = __builtin_amdgcn_sdot4(fb[l].z, 0x01010101, sacc, false);
              sacc = __builtin_amdgcn_sdot4(fb[l].w, 0x01010101, sacc, false);
              rs[l][pf] = sacc;
            }
          }
#pragma unroll
          for (int la = 0; la < L; ++la)
#pragma unroll
            for (int lw = 0; lw < LW; ++lw)
              if (la + lw >= SMIN)
                acc[la + lw - SMIN][pf] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wreg[tap % 3][lw], fb[la],
                                                                                 acc[la + lw - SMIN][pf], 0, 0, 0);
        }
        if constexpr (OFF) {  // pin the digit sums to their tap: sunk below the loop's branches, they would keep
                              // every tap's fragments alive (scratch)
#pragma unroll
          for (int pf = 0; pf < NPF; ++pf) asm volatile("" : "+v"(rs[0][pf]), "+v"(rs[1][pf]), "+v"(rs[2][pf]));
        }
      }
      if (NST == 1 && more) {  // one stage: refill it once every wave has read this chunk
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (last) tile_src(tn);
#pragma unroll
        for (int k = 0; k < PSL; ++k) issue(k, 0u, soffn);
      }
    }
    if constexpr (OFF) {  // weight = code + offset: + offset[c] * (window digit sum, all 9 cg of the group)
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int pf = 0; pf < NPF; ++pf) {
          int sacc = rs[l][pf];
          sacc += __shfl_xor(sacc, 16, kWave);
          sacc += __shfl_xor(sacc, 32, kWave);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[l][pf][r] += cor[r] * sacc;
        }
    }

    // ---- epilogue (conv_grouped.hip's) --------------------------------------------------------------
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
  if (a.yq) {
    const bool ovf = LEAN ? vmax > qmax : rintf(__fmul_rn(vmax, a.yq_inv)) > qmax;
    if (__any(ovf) && lane == 0) atomicMax(a.overflow, 1);
  }
}

template <int LW, bool OFF, int STRIDE, bool LEAN>
int launch_wide_one(const GroupedArgs& a, hipStream_t stream) {
  constexpr int lds_bytes = wide_stages(STRIDE) * wide_pieces(STRIDE) * 1024;
  static_assert(2 * lds_bytes <= 160 * 1024, "two workgroups per CU");
  const int gx = a.cout / 64;
  // about four (stride 1) or two (stride 2: 55 KiB of LDS each) workgroups per CU in all; each walks tiles from there
  int gy = ((STRIDE == 1 ? 1024 : 512) + gx - 1) / gx;
  if (gy > a.tiles) gy = a.tiles;
  hipLaunchKernelGGL((qconv_grouped_wide_kernel<LW, OFF, STRIDE, LEAN>), dim3(gx, gy), dim3(64 * kWWaves), lds_bytes,
                     stream, a);
  return check_hip(hipGetLastError(), "qconv_grouped_wide_kernel launch");
}

template <int LW, bool OFF>
int launch_wide_s(const GroupedArgs& a, int stride, bool lean, hipStream_t s) {
  if (stride == 1) return lean ? launch_wide_one<LW, OFF, 1, true>(a, s) : launch_wide_one<LW, OFF, 1, false>(a, s);
  return lean ? launch_wide_one<LW, OFF, 2, true>(a, s) : launch_wide_one<LW, OFF, 2, false>(a, s);
}

}  // namespace

bool grouped_wide_shape(int cg, int og) { return cg >= 128 && cg % 64 == 0 && og > 0 && og % 64 == 0; }

// a: as smpq_conv2d_grouped_fwd_q fills it for a geometry smpq_conv2d_grouped_supported takes
int launch_grouped_wide(const GroupedArgs& a, int wlimbs, int stride, bool lean, hipStream_t s) {
  if (wlimbs == 3) return launch_wide_s<3, false>(a, stride, lean, s);
  return a.w_off ? launch_wide_s<1, true>(a, stride, lean, s) : launch_wide_s<1, false>(a, stride, lean, s);
}

}  // namespace smpq
