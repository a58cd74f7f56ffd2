// Dilated narrow-channel 3x3 quantized conv (groups 1, stride 1, padding = dilation = d in {2, 4, 8},
// cin % 16 == 0 but cin % 64 != 0, cout % 16 == 0) for gfx950 on v_mfma_i32_16x16x64_i8: the conv2 of a
// Bottleneck built with width_per_group != 64 AND replace_stride_with_dilation, eval BatchNorm and
// ReLU folded in, on 3 activation limbs and 1 or 3 weight limbs. It joins the two parent kernels:
//
// Phase lattices (conv_dilated.hip). Output pixel (ph + d i, pw + d j) reads lattice pixels
// (i + kr - 1, j + kc - 1) of its own phase (ph, pw) only, zero outside 0 <= i' < LH(ph) =
// ceil((h - ph) / d), 0 <= j' < LW(pw) = ceil((w - pw) / d): the conv is d * d ordinary 3x3 / pad 1 /
// stride 1 convs, and a 10 x 10 halo patch of LATTICE pixels staged once serves all nine taps of an
// 8 x 8 lattice tile. The staged bytes per output do not grow with d.
//
// K in 16-byte chunks over channel slabs (conv_narrow.hip). That patch has exactly the pixel geometry
// of the narrow kernel's 3x3 / stride-1 patch, so the slab split, the padded pixel / row pitches and
// the conflict-free fragment reads are narrow_geo(cin, 3, 1) of conv_common.h, K within a slab is
// [tap][chunk] with a zero-padded last step, and the weights are the fragment-ordered copy of
// smpq_weights_narrow_expand(..., 3, 3, 1), read unchanged: no weight format of its own.
//
// Work split. A workgroup is 4 waves = 4 adjacent 16-output-channel fragments (blockIdx.x) and walks
// items (image, phase, 8 x 8 lattice tile) from blockIdx.y in steps of gridDim.y. Every phase gets the
// tile count of the largest lattice (phase 0); an item whose tile lies outside its own phase's lattice
// (smaller extents when d does not divide h or w, no pixel at all when ph >= h) is skipped before any
// DMA or barrier, which is workgroup-uniform because the item depends on blockIdx alone.
//
// Staging. Per item and slab the workgroup stages the slab's channels of the 10 x 10 lattice patch
// for the three limb planes by LDS-DMA (lds_dma.h dma16) as [limb][patch row][pixel][chunk]: piece p
// is LDS bytes [1024 p, + 1024), lane i its 16-B slot 64 p + i, whose source is lattice pixel
// (i0 - 1 + pr, j0 - 1 + pc) = input pixel (ph + d (i0 - 1 + pr), pw + d (j0 - 1 + pc)): the sources
// step d * cin along a lattice row and d * w * cin between rows. A position outside the phase's
// lattice, and the pitch padding, get the out-of-range buffer offset, which the DMA stages as zero.
//
// Weights. A wave owns one fragment; a step's codes are one coalesced KiB per weight plane, loaded
// straight into registers: resident for the whole item walk where the fragment is 3, 5 or 7 steps
// (cin 16, 32, 48: at most 3 planes x 7 steps = 84 VGPRs), otherwise streamed one step ahead.
//
// Weight offsets (one weight limb: weight = code + offset[c]): one MFMA per activation limb of the
// copy's all-ones plane gives the window digit sums in the accumulator layout; out-of-lattice taps
// were staged as zero and drop out on their own.
//
// Epilogue: conv_common.h / lds_dma.h arithmetic (limb_smin / limb_nacc passes, lean_v1, affine,
// lean_quad, encode4), so a value is rounded as the dense kernels round it: the lean static-range
// form when only limb planes are wanted, the general form (fp32 y, y_absmax, limb planes) otherwise.
// No residual. A wave's four pixel fragments are the tile's row pairs; after the lane-group transpose
// a lattice pixel's 16 channels of one limb plane go out in one 16-B store, at pixel pitch d * cout.
// Every global access of a tensor goes through a range-checked buffer resource with 32-bit offsets.
#include "lds_dma.h"

namespace smpq {
namespace {

constexpr int kXT = kNarrowTile;  // lattice tile edge
constexpr int kXWaves = 4;        // fragments per workgroup
constexpr long long kXBytesMax = 0x7fffff00LL;

struct NarrowDilatedArgs {
  const int8_t* xq;       // [3][n][h][w][cin]
  long long plane;        // bytes per activation limb plane
  const float* x_absmax;  // [n]
  const int8_t* wexp;     // [planes][nfrag][nk][64][16] fragment-ordered codes (+ the all-ones plane)
  long long wbytes;
  const int32_t* w_off;   // [cout] or NULL
  const float* col_scale;
  const float* col_shift;
  float* y;
  float* y_absmax;
  int8_t* yq;
  int32_t* overflow;
  float yq_inv, inv_qmax;
  int n, h, w, cin, cout, d, nfrag, relu;
  int ntw, ntile, tiles_img, tiles;  // column tiles, tiles of one phase, items of one image, of the batch
  NarrowGeo g;                       // narrow_geo(cin, 3, 1)
};

// LW weight limbs (1 or 3), OFF: weight offsets (LW == 1), LEAN: the static-range limb-plane
// epilogue, NKR: steps of the resident form (0: streaming)
template <int LW, bool OFF, bool LEAN, int NKR>
__global__ __launch_bounds__(64 * kXWaves) void qconv_narrow_dilated_kernel(NarrowDilatedArgs a) {
  constexpr int L = 3;
  constexpr int SMIN = limb_smin(L, LW), NACC = limb_nacc(L, LW);
  constexpr int WP = LW + (OFF ? 1 : 0);  // weight planes held (the last one: all ones on the real K)
  constexpr int NPF = kXT * kXT / 16;     // pixel fragments of a tile
  constexpr int PW = kXT + 2;             // patch edge in lattice pixels
  static_assert(NPF == 4, "the limb-plane stores transpose four pixel fragments");
  static_assert(!OFF || LW == 1, "weight offsets come with one weight limb");
  extern __shared__ __attribute__((aligned(1024))) int8_t lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int frow = lane & 15, grp = lane >> 4;
  const int f = blockIdx.x * kXWaves + wave;
  const bool active = f < a.nfrag;
  const int fr = active ? f : 0;
  const NarrowGeo& g = a.g;
  const int pp = g.pp, rp = g.rp, d = a.d;
  const int plimb = PW * rp * 16;  // LDS bytes per limb
  const int slots = L * PW * rp;   // 16-B slots of the patch image, padding included
  const int pieces = (slots + 63) / 64;

  const v4i xrs = make_rsrc(a.xq, (long long)L * a.plane);
  const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(a.wexp), 0, (int)a.wbytes, 0x00020000);
  const unsigned wplane = (unsigned)a.nfrag * (unsigned)g.nk * 1024u;
  const unsigned wfrag = (unsigned)fr * (unsigned)g.nk * 1024u + (unsigned)lane * 16u;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds));
  const long long oplane = (long long)a.n * a.h * a.w * a.cout;  // elements per output plane (ho = h, wo = w)
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y ? (int)(4 * oplane) : 0, 0x00020000);
  const auto qrs = __builtin_amdgcn_make_buffer_rsrc(a.yq, 0, a.yq ? (int)(L * oplane) : 0, 0x00020000);

  // ---- resident form: this wave's fragment, kept in registers for every item ----------------------
  v4i wreg[NKR ? NKR : 1][WP];
  int tapoff[NKR ? NKR : 1];
  if constexpr (NKR > 0) {
#pragma unroll
    for (int j = 0; j < NKR; ++j) {
#pragma unroll
      for (int p = 0; p < WP; ++p)
        wreg[j][p] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrs, wfrag + p * wplane + j * 1024u, 0, 0));
      tapoff[j] = 16 * narrow_tap(4 * j + grp, g.cs, 9, pp, rp);
    }
  }
  int pixoff[NPF];
#pragma unroll
  for (int pf = 0; pf < NPF; ++pf) pixoff[pf] = 16 * narrow_pix(frow, pf, 1, pp, rp);

  const int c4 = 16 * fr + 4 * grp;  // this lane's 4 output channels
  const float4 cs = *reinterpret_cast<const float4*>(a.col_scale + c4);
  const float4 csh = *reinterpret_cast<const float4*>(a.col_shift + c4);
  int cor[4] = {0, 0, 0, 0};
  if constexpr (OFF) {
    const int4 o = *reinterpret_cast<const int4*>(a.w_off + c4);
    cor[0] = o.x, cor[1] = o.y, cor[2] = o.z, cor[3] = o.w;
  }
  constexpr float qmax = act_qmax<L>();
  const bool relu = a.relu != 0;
  float vmax = 0.f;  // LEAN: the largest rounded code; otherwise max |y| (both over every item)
  bool first = true;

  for (int t = blockIdx.y; t < a.tiles; t += gridDim.y) {
    const int img = t / a.tiles_img, rem = t - img * a.tiles_img;
    const int phase = rem / a.ntile, tl = rem - phase * a.ntile;
    const int ph = phase / d, pw = phase - ph * d;
    const int tr = tl / a.ntw, tc = tl - tr * a.ntw;
    const int i0 = tr * kXT, j0 = tc * kXT;
    // this phase's lattice (no row at all when ph >= h)
    const int lh = (a.h - ph + d - 1) / d, lw = (a.w - pw + d - 1) / d;
    if (i0 >= lh || j0 >= lw) continue;  // (workgroup-uniform, before any DMA or barrier)
    const int pix0 = (img * a.h + ph) * a.w + pw;  // input = output pixel of lattice position (0, 0)

    v4i acc[NACC][NPF], gs[OFF ? L : 1][NPF];
#pragma unroll
    for (int pf = 0; pf < NPF; ++pf) {
#pragma unroll
      for (int s = 0; s < NACC; ++s) acc[s][pf] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int l = 0; l < (OFF ? L : 1); ++l) gs[l][pf] = v4i{0, 0, 0, 0};
    }

    for (int s = 0; s < g.nslab; ++s) {
      const int cwc = s == g.nslab - 1 ? g.cl : g.cs;  // chunks of this slab
      const int c_lo = 16 * s * g.cs;
      if (!first) {  // every wave is done with the last patch
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      first = false;
      // ---- stage the lattice patch: piece p = LDS bytes [1024 p, + 1024), lane i its slot 64 p + i ----
      for (int p = wave; p < pieces; p += kXWaves) {
        const int q = 64 * p + lane;
        const int l = q / (PW * rp), r1 = q - l * (PW * rp);
        const int pr = r1 / rp, r2 = r1 - pr * rp;
        const int pc = r2 / pp, ch = r2 - pc * pp;
        const int li = i0 - 1 + pr, lj = j0 - 1 + pc;  // lattice pixel
        unsigned src = kOOB;
        if (q < slots && pc < PW && ch < cwc && (unsigned)li < (unsigned)lh && (unsigned)lj < (unsigned)lw)
          src = (unsigned)(l * a.plane + ((long long)pix0 + (long long)d * (li * a.w + lj)) * a.cin + c_lo + 16 * ch);
        dma16(__builtin_amdgcn_readfirstlane(lds0 + (unsigned)p * 1024u), xrs, src, 0u);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (!active) continue;  // (wave-uniform; the barriers above are reached by every wave)

      // ---- all taps of the slab out of LDS ---------------------------------------------------------
      if constexpr (NKR > 0) {
#pragma unroll
        for (int j = 0; j < NKR; ++j) narrow_step<LW, OFF, NACC, SMIN>(lds, plimb, pixoff, tapoff[j], wreg[j], acc, gs);
      } else {
        const int nks = (9 * cwc + 3) / 4;
        const unsigned wslab = wfrag + (unsigned)(s * g.nkf) * 1024u;
        v4i wcur[WP], wnxt[WP];
#pragma unroll
        for (int p = 0; p < WP; ++p)
          wcur[p] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrs, wslab + p * wplane, 0, 0));
        for (int j = 0; j < nks; ++j) {
          // (the step past the slab's last one is loaded from an out-of-range offset: zeros, unused)
          const unsigned wn = j + 1 < nks ? wslab + (unsigned)(j + 1) * 1024u : kOOB;
#pragma unroll
          for (int p = 0; p < WP; ++p)
            wnxt[p] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrs, wn == kOOB ? kOOB : wn + p * wplane, 0, 0));
          narrow_step<LW, OFF, NACC, SMIN>(lds, plimb, pixoff, 16 * narrow_tap(4 * j + grp, cwc, 9, pp, rp), wcur, acc, gs);
#pragma unroll
          for (int p = 0; p < WP; ++p) wcur[p] = wnxt[p];
        }
      }
    }
    if (!active) continue;
    if constexpr (OFF) {  // weight = code + offset: + offset[c] * (window digit sum over the real K)
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int pf = 0; pf < NPF; ++pf)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[l][pf][r] += cor[r] * gs[l][pf][r];
    }

    // ---- epilogue: lattice pixel (i0 + 2 pf + (frow >> 3), j0 + (frow & 7)) of fragment pf ----------
    const float rscale = a.x_absmax[img] * a.inv_qmax;
    const float inv = a.yq_inv;
    const int ljq = j0 + (frow & 7);
    // lane group g stores pixel fragment g: its 16 channels, 16 B per limb
    const int liq = i0 + 2 * grp + (frow >> 3);
    const bool okq = liq < lh && ljq < lw;
    const unsigned qo = (unsigned)(((long long)pix0 + (long long)d * (liq * a.w + ljq)) * a.cout + 16 * f);
    unsigned wq[NPF][L];
    float amax = 0.f;
#pragma unroll
    for (int pf = 0; pf < NPF; ++pf) {
      const int li = i0 + 2 * pf + (frow >> 3);
      const bool ok = li < lh && ljq < lw;
      v4i accq[NACC];
#pragma unroll
      for (int s = 0; s < NACC; ++s) accq[s] = acc[s][pf];
      if constexpr (LEAN) {
        const float csq[4] = {cs.x * inv, cs.y * inv, cs.z * inv, cs.w * inv};
        const float shq[4] = {csh.x * inv, csh.y * inv, csh.z * inv, csh.w * inv};
        const int none[4] = {0, 0, 0, 0};
        const float m = lean_quad<L, NACC, SMIN>(accq, rscale, csq, shq, false, none, 0.f, relu, relu ? 0.f : -qmax, wq[pf]);
        vmax = ok ? fmaxf(vmax, m) : vmax;
      } else {
        const float csr[4] = {cs.x, cs.y, cs.z, cs.w}, shr[4] = {csh.x, csh.y, csh.z, csh.w};
        const unsigned eo = (unsigned)(((long long)pix0 + (long long)d * (li * a.w + ljq)) * a.cout + c4);
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
#pragma unroll
      for (int l = 0; l < L; ++l) {
        unsigned w0 = wq[0][l], w1 = wq[1][l], w2 = wq[2][l], w3 = wq[3][l];
        transpose4(w0, w1, w2, w3);
        __builtin_amdgcn_raw_buffer_store_b128(v4u{w0, w1, w2, w3}, qrs, okq ? qo + (unsigned)(l * oplane) : kOOB, 0, 0);
      }
    }
  }
  if (a.yq && active) {
    const bool ovf = LEAN ? vmax > qmax : rintf(__fmul_rn(vmax, a.yq_inv)) > qmax;
    if (__any(ovf) && lane == 0) atomicMax(a.overflow, 1);
  }
}

template <int LW, bool OFF, bool LEAN, int NKR>
int launch_nd_one(const NarrowDilatedArgs& a, hipStream_t stream) {
  const auto fn = qconv_narrow_dilated_kernel<LW, OFF, LEAN, NKR>;
  static const hipError_t attr = [&] {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kNarrowLdsMax);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  }();
  if (attr != hipSuccess) return check_hip(attr, "qconv_narrow_dilated_kernel LDS attribute");
  const int gx = (a.nfrag + kXWaves - 1) / kXWaves;
  int gy = (1024 + gx - 1) / gx;  // about four workgroups per CU in all; each walks items from there
  if (gy > a.tiles) gy = a.tiles;
  hipLaunchKernelGGL(fn, dim3(gx, gy), dim3(64 * kXWaves), a.g.lds_bytes, stream, a);
  return check_hip(hipGetLastError(), "qconv_narrow_dilated_kernel launch");
}

template <int LW, bool OFF, bool LEAN>
int launch_nd_k(const NarrowDilatedArgs& a, hipStream_t s) {
  switch (narrow_resident_steps(a.g)) {  // 3x3: cin 16, 32, 48
    case 3: return launch_nd_one<LW, OFF, LEAN, 3>(a, s);
    case 5: return launch_nd_one<LW, OFF, LEAN, 5>(a, s);
    case 7: return launch_nd_one<LW, OFF, LEAN, 7>(a, s);
    default: return launch_nd_one<LW, OFF, LEAN, 0>(a, s);
  }
}

template <int LW, bool OFF>
int launch_nd_w(const NarrowDilatedArgs& a, bool lean, hipStream_t s) {
  return lean ? launch_nd_k<LW, OFF, true>(a, s) : launch_nd_k<LW, OFF, false>(a, s);
}

bool narrow_dilated_supported(int cin, int cout, int kh, int kw, int stride, int pad, int dilation, int limbs,
                              int wlimbs) {
  if (kh != 3 || kw != 3 || stride != 1 || pad != dilation || (dilation != 2 && dilation != 4 && dilation != 8))
    return false;
  if (cin <= 0 || cout <= 0 || cin % 16 != 0 || cin % 64 == 0 || cout % 16 != 0) return false;
  if (limbs != 3 || (wlimbs != 1 && wlimbs != 3)) return false;
  NarrowGeo g;
  return narrow_geo(cin, 3, 1, g);
}

}  // namespace
}  // namespace smpq

using namespace smpq;

extern "C" int smpq_conv2d_narrow_dilated_supported(int cin, int cout, int kh, int kw, int stride, int pad,
                                                    int dilation, int limbs, int wlimbs) {
  return narrow_dilated_supported(cin, cout, kh, kw, stride, pad, dilation, limbs, wlimbs) ? 1 : 0;
}

extern "C" int smpq_conv2d_narrow_dilated_fwd_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                                const int8_t* codes, const int8_t* codes_expanded, int wlimbs,
                                                const int32_t* offset, int cout, int kh, int kw, int stride, int pad,
                                                int dilation, const float* col_scale, const float* col_shift, int relu,
                                                int limbs, float* y, float* y_absmax, int8_t* yq, float yq_range,
                                                int32_t* overflow, smpq_stream_t stream) {
  if (!xq || !x_absmax || !codes || !codes_expanded || !col_scale || !col_shift || (!y && !yq))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_dilated_fwd_q: null pointer");
  if (yq && (!overflow || !(yq_range > 0.f)))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_dilated_fwd_q: yq needs overflow flag and a positive range");
  if (limbs != 3 || (wlimbs != 1 && wlimbs != 3))
    return fail(SMPQ_E_INVALID,
                "smpq_conv2d_narrow_dilated_fwd_q: built for 3 activation limbs and 1 or 3 weight limbs");
  if (n <= 0 || h <= 0 || w <= 0) return fail(SMPQ_E_SHAPE, "smpq_conv2d_narrow_dilated_fwd_q: bad shape");
  NarrowDilatedArgs a = {};
  if (!narrow_dilated_supported(cin, cout, kh, kw, stride, pad, dilation, limbs, wlimbs) || !narrow_geo(cin, 3, 1, a.g))
    return fail(SMPQ_E_SHAPE,
                "smpq_conv2d_narrow_dilated_fwd_q: unsupported geometry (smpq_conv2d_narrow_dilated_supported: dense, "
                "3x3 / stride 1 / pad == dilation in {2, 4, 8}, cin % 16 == 0 and cin % 64 != 0, cout % 16 == 0)");
  if ((((uintptr_t)xq | (uintptr_t)codes_expanded | (uintptr_t)col_scale | (uintptr_t)col_shift | (uintptr_t)offset |
        (uintptr_t)y | (uintptr_t)yq) & 15) != 0)
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_dilated_fwd_q: operands must be 16-B aligned");
  a.plane = (long long)n * h * w * cin;
  a.wbytes = narrow_expand_bytes(wlimbs, cout, a.g);
  const long long oplane = (long long)n * h * w * cout;  // stride 1, pad == dilation: ho = h, wo = w
  // 32-bit buffer offsets over all three limb planes (and the fp32 output): the caller splits the batch
  if (3 * a.plane > kXBytesMax || (yq && 3 * oplane > kXBytesMax) || (y && 4 * oplane > kXBytesMax) ||
      a.wbytes > kXBytesMax)
    return fail(SMPQ_E_SHAPE, "smpq_conv2d_narrow_dilated_fwd_q: a tensor of 2 GiB or more (split the batch)");
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
  a.n = n, a.h = h, a.w = w, a.cin = cin, a.cout = cout, a.d = dilation;
  a.nfrag = cout / 16, a.relu = relu ? 1 : 0;
  // every phase gets the tiles of the largest lattice (phase 0)
  const int lh = (h + dilation - 1) / dilation, lw = (w + dilation - 1) / dilation;
  a.ntw = (lw + kXT - 1) / kXT;
  a.ntile = ((lh + kXT - 1) / kXT) * a.ntw;
  a.tiles_img = dilation * dilation * a.ntile;
  if ((long long)n * a.tiles_img > 0x7fffffffLL)
    return fail(SMPQ_E_SHAPE, "smpq_conv2d_narrow_dilated_fwd_q: too many tiles");
  a.tiles = n * a.tiles_img;
  const bool lean = yq && !y && !y_absmax;
  hipStream_t s = (hipStream_t)stream;
  if (wlimbs == 3) return launch_nd_w<3, false>(a, lean, s);
  return a.w_off ? launch_nd_w<1, true>(a, lean, s) : launch_nd_w<1, false>(a, lean, s);
}
