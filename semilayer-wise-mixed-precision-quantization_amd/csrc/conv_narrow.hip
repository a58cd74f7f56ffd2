// Narrow-channel dense quantized conv (groups 1, dilation 1) for gfx950 on v_mfma_i32_16x16x64_i8:
// cin % 16 == 0 but cin % 64 != 0, cout % 16 == 0; 3x3 / pad 1 / stride 1 or 2 (the conv2 of a
// Bottleneck built with width_per_group != 64, resnet.py:75-78) and 1x1 / pad 0 / stride 1 (its
// conv3), with eval BatchNorm, the identity add and ReLU folded in, on 3 activation limbs and 1 or 3
// weight limbs.
//
// K in 16-byte chunks. One lane's 16 K bytes of the MFMA are one 16-channel chunk of one tap of one
// pixel, so K needs no multiple of 64 channels: within a channel slab of cwc chunks K is ordered
// [tap][chunk], chunk kk = 4 j + (lane >> 4) of step j is tap kk / cwc, channels 16 (kk % cwc) .. + 15
// of the slab, and the last step of a slab is padded with zero codes: ceil(taps * cwc / 4) steps.
//
// Channel slabs. The patch of all channels need not fit LDS (17 x 17 pixels at stride 2), so the
// channels are cut into slabs of cs chunks (narrow_geo: the widest slab whose padded patch fits 160
// KB; the last slab takes what is left), walked in order for every tile with the accumulators kept.
// The fragment-ordered weight copy ([plane][cout / 16][NK][64 lanes][16 B], smpq_weights_narrow_expand)
// follows the same order: the steps of slab 0, then those of slab 1, ...
//
// Weights. A wave owns one 16-output-channel fragment; a step's codes are one coalesced KiB per weight
// plane, loaded straight into registers. Resident form (NKR > 0): one slab of exactly NKR in {1, 2, 3,
// 5, 7} steps, the fragment is loaded once and kept for every tile (all 1x1 convs up to cin 112 and
// the 3x3 ones at cin 16, 32, 48: at most 3 planes x 7 steps = 84 VGPRs). Streaming form (NKR == 0):
// anything else; the codes of step j + 1 are loaded while step j runs.
//
// Activations. A workgroup is 4 waves = 4 adjacent fragments and walks 8 x 8 output tiles (blockIdx.y,
// + gridDim.y, ...). Per tile and slab it stages, once for all taps, the (7 stride + 3)^2 input pixels
// (8 x 8 for 1x1) of the slab's channels for the three limb planes by LDS-DMA (lds_dma.h dma16) as
// [limb][patch row][pixel][chunk] with a pixel pitch of PP and a row pitch of RP chunks (narrow_geo
// pads both: tools/narrow_conflicts.py); positions outside the image, and the padding, get an
// out-of-range buffer offset, which the DMA stages as zero. A wave's four pixel fragments are the
// tile's row pairs, so a lane ends with 4 consecutive output channels of 4 pixels.
//
// Weight offsets (one weight limb: weight = code + offset[c]): the expanded copy carries one more
// plane that is 1 on the real K and 0 on the padding; one MFMA of it per activation limb gives the
// window digit sums in the accumulator layout.
//
// Epilogue: conv_common.h / lds_dma.h arithmetic (limb_smin / limb_nacc passes, lean_v1, affine,
// lean_quad, encode4, decode4), so a value is rounded as the dense kernels round it, with the residual
// as fp32 NHWC (general form) or as limb planes + range (both forms). Every global access of a tensor
// goes through a range-checked buffer resource with 32-bit offsets.
#include "lds_dma.h"

namespace smpq {
namespace {

// (the slab geometry, the fragment-read offsets and the K step are in conv_common.h: conv_narrow_dilated.hip
// runs its phase lattices on them)
constexpr int kNT = kNarrowTile;         // output tile edge
constexpr int kNWaves = 4;               // fragments per workgroup
constexpr int kNLdsMax = kNarrowLdsMax;  // LDS per workgroup on gfx950
constexpr long long kNBytesMax = 0x7fffff00LL;

struct NarrowArgs {
  const int8_t* xq;       // [3][n][h][w][cin]
  long long plane;        // bytes per activation limb plane
  const float* x_absmax;  // [n]
  const int8_t* wexp;     // [planes][nfrag][nk][64][16] fragment-ordered codes (+ the all-ones plane)
  long long wbytes;
  const int32_t* w_off;   // [cout] or NULL
  const float* col_scale;
  const float* col_shift;
  const float* residual;  // fp32 NHWC or NULL
  const int8_t* res_q;    // [3][n][ho][wo][cout] or NULL
  float res_scale;
  float* y;
  float* y_absmax;
  int8_t* yq;
  int32_t* overflow;
  float yq_inv, inv_qmax;
  int n, h, w, cin, cout, ho, wo, nfrag, relu, stride, pad;
  int ntw, tiles_img, tiles;
  NarrowGeo g;
};

bool narrow_shape_ok(int cin, int cout, int kh, int kw, int stride, int pad) {
  if (cin <= 0 || cout <= 0 || cin % 16 != 0 || cin % 64 == 0 || cout % 16 != 0) return false;
  if (kh == 3 && kw == 3) return pad == 1 && (stride == 1 || stride == 2);
  return kh == 1 && kw == 1 && pad == 0 && stride == 1;
}

bool narrow_supported(int cin, int cout, int kh, int kw, int stride, int pad, int limbs, int wlimbs) {
  if (limbs != 3 || (wlimbs != 1 && wlimbs != 3) || !narrow_shape_ok(cin, cout, kh, kw, stride, pad)) return false;
  NarrowGeo g;
  return narrow_geo(cin, kh, stride, g);
}

// LW weight limbs (1 or 3), OFF: weight offsets (LW == 1), LEAN: the static-range limb-plane
// epilogue, NKR: steps of the resident form (0: streaming)
template <int LW, bool OFF, bool LEAN, int NKR>
__global__ __launch_bounds__(64 * kNWaves) void qconv_narrow_kernel(NarrowArgs a) {
  constexpr int L = 3;
  constexpr int SMIN = limb_smin(L, LW), NACC = limb_nacc(L, LW);
  constexpr int WP = LW + (OFF ? 1 : 0);  // weight planes held (the last one: all ones on the real K)
  constexpr int NPF = kNT * kNT / 16;     // pixel fragments of a tile
  static_assert(NPF == 4, "the limb-plane stores transpose four pixel fragments");
  extern __shared__ __attribute__((aligned(1024))) int8_t lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int frow = lane & 15, grp = lane >> 4;
  const int f = blockIdx.x * kNWaves + wave;
  const bool active = f < a.nfrag;
  const int fr = active ? f : 0;
  const NarrowGeo& g = a.g;
  const int pw = g.pw, pp = g.pp, rp = g.rp, stride = a.stride;
  const int plimb = pw * rp * 16;    // LDS bytes per limb
  const int slots = L * pw * rp;     // 16-B slots of the patch image, padding included
  const int pieces = (slots + 63) / 64;

  const v4i xrs = make_rsrc(a.xq, (long long)L * a.plane);
  const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(a.wexp), 0, (int)a.wbytes, 0x00020000);
  const unsigned wplane = (unsigned)a.nfrag * (unsigned)g.nk * 1024u;
  const unsigned wfrag = (unsigned)fr * (unsigned)g.nk * 1024u + (unsigned)lane * 16u;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds));
  const long long oplane = (long long)a.n * a.ho * a.wo * a.cout;  // elements per output plane
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y ? (int)(4 * oplane) : 0, 0x00020000);
  const auto qrs = __builtin_amdgcn_make_buffer_rsrc(a.yq, 0, a.yq ? (int)(L * oplane) : 0, 0x00020000);
  const auto rfs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.residual), 0,
                                                     a.residual ? (int)(4 * oplane) : 0, 0x00020000);
  const auto rqs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(a.res_q), 0,
                                                     a.res_q ? (int)(L * oplane) : 0, 0x00020000);
  const bool has_rq = a.res_q != nullptr;

  // ---- resident form: this wave's fragment, kept in registers for every tile --------------------
  v4i wreg[NKR ? NKR : 1][WP];
  int tapoff[NKR ? NKR : 1];
  if constexpr (NKR > 0) {
#pragma unroll
    for (int j = 0; j < NKR; ++j) {
#pragma unroll
      for (int p = 0; p < WP; ++p)
        wreg[j][p] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrs, wfrag + p * wplane + j * 1024u, 0, 0));
      tapoff[j] = 16 * narrow_tap(4 * j + grp, g.cs, g.taps, pp, rp);
    }
  }
  int pixoff[NPF];
#pragma unroll
  for (int pf = 0; pf < NPF; ++pf) pixoff[pf] = 16 * narrow_pix(frow, pf, stride, pp, rp);

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
  float vmax = 0.f;  // LEAN: the largest rounded code; otherwise max |y| (both over every tile)
  bool first = true;

  for (int t = blockIdx.y; t < a.tiles; t += gridDim.y) {
    const int img = t / a.tiles_img, rem = t - img * a.tiles_img;
    const int tr = rem / a.ntw, tc = rem - tr * a.ntw;
    const int oh0 = tr * kNT, ow0 = tc * kNT;
    const int ih0 = oh0 * stride - a.pad, iw0 = ow0 * stride - a.pad;
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
      // ---- stage the patch: piece p = LDS bytes [1024 p, + 1024), lane i its slot 64 p + i ----------
      for (int p = wave; p < pieces; p += kNWaves) {
        const int q = 64 * p + lane;
        const int l = q / (pw * rp), r1 = q - l * (pw * rp);
        const int pr = r1 / rp, r2 = r1 - pr * rp;
        const int pc = r2 / pp, ch = r2 - pc * pp;
        const int ih = ih0 + pr, iw = iw0 + pc;
        unsigned src = kOOB;
        if (q < slots && pc < pw && ch < cwc && (unsigned)ih < (unsigned)a.h && (unsigned)iw < (unsigned)a.w)
          src = (unsigned)(l * a.plane + ((long long)(img * a.h + ih) * a.w + iw) * a.cin + c_lo + 16 * ch);
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
        const int nks = (g.taps * cwc + 3) / 4;
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
          narrow_step<LW, OFF, NACC, SMIN>(lds, plimb, pixoff, 16 * narrow_tap(4 * j + grp, cwc, g.taps, pp, rp), wcur,
                                           acc, gs);
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

    // ---- epilogue ---------------------------------------------------------------------------------
    const float rscale = a.x_absmax[img] * a.inv_qmax;
    const float inv = a.yq_inv;
    // lane group g stores (and reads the residual of) pixel fragment g: its 16 channels, 16 B per limb
    const int ohq = oh0 + 2 * grp + (frow >> 3), owq = ow0 + (frow & 7);
    const bool okq = ohq < a.ho && owq < a.wo;
    const unsigned qo = (unsigned)(((long long)(img * a.ho + ohq) * a.wo + owq) * a.cout + 16 * f);
    int rqv[NPF][4];
    if (has_rq) {
      unsigned rw[NPF][L];
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rqs, okq ? qo + (unsigned)(l * oplane) : kOOB, 0, 0);
        unsigned w0 = v[0], w1 = v[1], w2 = v[2], w3 = v[3];
        transpose4(w0, w1, w2, w3);  // -> the lane's 4 channels of pixel fragments 0 .. 3
        rw[0][l] = w0, rw[1][l] = w1, rw[2][l] = w2, rw[3][l] = w3;
      }
#pragma unroll
      for (int pf = 0; pf < NPF; ++pf) decode4<L>(rw[pf], rqv[pf]);
    } else {
#pragma unroll
      for (int pf = 0; pf < NPF; ++pf)
#pragma unroll
        for (int r = 0; r < 4; ++r) rqv[pf][r] = 0;
    }
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
        const float m = lean_quad<L, NACC, SMIN>(accq, rscale, csq, shq, has_rq, rqv[pf], a.res_scale * inv, relu,
                                                 relu ? 0.f : -qmax, wq[pf]);
        vmax = ok ? fmaxf(vmax, m) : vmax;
      } else {
        const float csr[4] = {cs.x, cs.y, cs.z, cs.w}, shr[4] = {csh.x, csh.y, csh.z, csh.w};
        const unsigned eo = (unsigned)(((long long)(img * a.ho + oh) * a.wo + ow) * a.cout + c4);
        v4u rv = {0u, 0u, 0u, 0u};
        if (a.residual && !has_rq) rv = __builtin_amdgcn_raw_buffer_load_b128(rfs, ok ? 4u * eo : kOOB, 0, 0);
        float o[4];
        float am = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[r] = affine(lean_v1<NACC, SMIN>(accq, r), rscale, csr[r], shr[r]);
          if (has_rq) o[r] = __fadd_rn(o[r], __fmul_rn(a.res_scale, (float)rqv[pf][r]));
          else if (a.residual) o[r] = __fadd_rn(o[r], __uint_as_float(rv[r]));
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
int launch_narrow_one(const NarrowArgs& a, hipStream_t stream) {
  const auto fn = qconv_narrow_kernel<LW, OFF, LEAN, NKR>;
  static const hipError_t attr = [&] {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kNLdsMax);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  }();
  if (attr != hipSuccess) return check_hip(attr, "qconv_narrow_kernel LDS attribute");
  const int gx = (a.nfrag + kNWaves - 1) / kNWaves;
  int gy = (1024 + gx - 1) / gx;  // about four workgroups per CU in all; each walks tiles from there
  if (gy > a.tiles) gy = a.tiles;
  hipLaunchKernelGGL(fn, dim3(gx, gy), dim3(64 * kNWaves), a.g.lds_bytes, stream, a);
  return check_hip(hipGetLastError(), "qconv_narrow_kernel launch");
}

template <int LW, bool OFF, bool LEAN>
int launch_narrow_k(const NarrowArgs& a, hipStream_t s) {
  switch (narrow_resident_steps(a.g)) {
    case 1: return launch_narrow_one<LW, OFF, LEAN, 1>(a, s);
    case 2: return launch_narrow_one<LW, OFF, LEAN, 2>(a, s);
    case 3: return launch_narrow_one<LW, OFF, LEAN, 3>(a, s);
    case 5: return launch_narrow_one<LW, OFF, LEAN, 5>(a, s);
    case 7: return launch_narrow_one<LW, OFF, LEAN, 7>(a, s);
    default: return launch_narrow_one<LW, OFF, LEAN, 0>(a, s);
  }
}

template <int LW, bool OFF>
int launch_narrow_w(const NarrowArgs& a, bool lean, hipStream_t s) {
  return lean ? launch_narrow_k<LW, OFF, true>(a, s) : launch_narrow_k<LW, OFF, false>(a, s);
}

// compact codes [wlimbs][cout][taps * cin] (k = tap * cin + ci) -> [planes][nfrag][nk][64 lanes][16 B],
// one byte per thread
__global__ void narrow_expand_kernel(const int8_t* __restrict__ codes, int wlimbs, int cout, int cin, NarrowGeo g,
                                     int8_t* __restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int nfrag = cout / 16;
  const int b = (int)(i & 15), lane = (int)((i >> 4) & 63);
  long long rest = i >> 10;
  const int jt = (int)(rest % g.nk);
  rest /= g.nk;
  const int f = (int)(rest % nfrag), p = (int)(rest / nfrag);
  int s = jt / g.nkf;
  s = s < g.nslab ? s : g.nslab - 1;
  const int j = jt - s * g.nkf, cwc = s == g.nslab - 1 ? g.cl : g.cs;
  const int row = 16 * f + (lane & 15), kk = 4 * j + (lane >> 4);
  const int tap = kk / cwc, sub = kk - tap * cwc;
  int v = 0;
  if (tap < g.taps) {
    const int ch = 16 * (s * g.cs + sub) + b;
    v = p < wlimbs ? codes[((long long)p * cout + row) * ((long long)g.taps * cin) + (long long)tap * cin + ch] : 1;
  }
  out[i] = (int8_t)v;
}

constexpr const char* kNarrowRule =
    "smpq_conv2d_narrow_supported: dense, cin % 16 == 0 and cin % 64 != 0, cout % 16 == 0, 3x3 / pad 1 / stride 1 or "
    "2 or 1x1 / pad 0 / stride 1, 3 activation limbs, 1 or 3 weight limbs";

}  // namespace
}  // namespace smpq

using namespace smpq;

extern "C" int smpq_conv2d_narrow_supported(int cin, int cout, int kh, int kw, int stride, int pad, int limbs,
                                            int wlimbs) {
  return narrow_supported(cin, cout, kh, kw, stride, pad, limbs, wlimbs) ? 1 : 0;
}

extern "C" size_t smpq_weights_narrow_expand_bytes(int wlimbs, int cout, int cin, int kh, int kw, int stride) {
  NarrowGeo g;
  if (!narrow_supported(cin, cout, kh, kw, stride, kh == 3 ? 1 : 0, 3, wlimbs) || !narrow_geo(cin, kh, stride, g)) return 0;
  const long long bytes = narrow_expand_bytes(wlimbs, cout, g);
  return bytes <= kNBytesMax ? (size_t)bytes : 0;
}

extern "C" int smpq_weights_narrow_expand(const int8_t* codes, int wlimbs, int cout, int cin, int kh, int kw,
                                          int stride, int8_t* out, smpq_stream_t stream) {
  if (!codes || !out) return fail(SMPQ_E_INVALID, "smpq_weights_narrow_expand: null pointer");
  if (((uintptr_t)out) & 15) return fail(SMPQ_E_INVALID, "smpq_weights_narrow_expand: out must be 16-B aligned");
  const long long total = (long long)smpq_weights_narrow_expand_bytes(wlimbs, cout, cin, kh, kw, stride);
  if (total == 0)
    return fail(SMPQ_E_SHAPE, std::string("smpq_weights_narrow_expand: not an operand the kernel takes (") + kNarrowRule + ")");
  NarrowGeo g;
  narrow_geo(cin, kh, stride, g);
  hipLaunchKernelGGL(narrow_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     codes, wlimbs, cout, cin, g, out, total);
  return check_hip(hipGetLastError(), "narrow_expand_kernel launch");
}

extern "C" int smpq_conv2d_narrow_fwd_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                        const int8_t* codes, const int8_t* codes_expanded, int wlimbs,
                                        const int32_t* offset, int cout, int kh, int kw, int stride, int pad,
                                        const float* col_scale, const float* col_shift, const float* residual,
                                        int relu, int limbs, float* y, float* y_absmax, int8_t* yq, float yq_range,
                                        int32_t* overflow, const int8_t* residual_q, float residual_range,
                                        smpq_stream_t stream) {
  if (!xq || !x_absmax || !codes || !codes_expanded || !col_scale || !col_shift || (!y && !yq))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_fwd_q: null pointer");
  if (yq && (!overflow || !(yq_range > 0.f)))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_fwd_q: yq needs overflow flag and a positive range");
  if (residual && residual_q) return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_fwd_q: two residuals");
  if (residual_q && !(residual_range > 0.f))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_fwd_q: residual_q needs a positive range");
  if (limbs != 3 || (wlimbs != 1 && wlimbs != 3))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_fwd_q: built for 3 activation limbs and 1 or 3 weight limbs");
  if (n <= 0 || h <= 0 || w <= 0) return fail(SMPQ_E_SHAPE, "smpq_conv2d_narrow_fwd_q: bad shape");
  NarrowArgs a = {};
  if (!narrow_supported(cin, cout, kh, kw, stride, pad, limbs, wlimbs) || !narrow_geo(cin, kh, stride, a.g))
    return fail(SMPQ_E_SHAPE, std::string("smpq_conv2d_narrow_fwd_q: unsupported geometry (") + kNarrowRule + ")");
  if ((((uintptr_t)xq | (uintptr_t)codes_expanded | (uintptr_t)col_scale | (uintptr_t)col_shift | (uintptr_t)offset |
        (uintptr_t)y | (uintptr_t)yq | (uintptr_t)residual | (uintptr_t)residual_q) & 15) != 0)
    return fail(SMPQ_E_INVALID, "smpq_conv2d_narrow_fwd_q: operands must be 16-B aligned");
  a.ho = (h + 2 * pad - kh) / stride + 1;
  a.wo = (w + 2 * pad - kw) / stride + 1;
  a.plane = (long long)n * h * w * cin;
  a.wbytes = narrow_expand_bytes(wlimbs, cout, a.g);
  const long long oplane = (long long)n * a.ho * a.wo * cout;
  // 32-bit buffer offsets over all three limb planes (and the fp32 tensors): the caller splits the batch
  if (3 * a.plane > kNBytesMax || ((yq || residual_q) && 3 * oplane > kNBytesMax) ||
      ((y || residual) && 4 * oplane > kNBytesMax) || a.wbytes > kNBytesMax)
    return fail(SMPQ_E_SHAPE, "smpq_conv2d_narrow_fwd_q: a tensor of 2 GiB or more (split the batch)");
  a.xq = xq;
  a.x_absmax = x_absmax;
  a.wexp = codes_expanded;
  a.w_off = wlimbs == 1 ? offset : nullptr;
  a.col_scale = col_scale;
  a.col_shift = col_shift;
  a.residual = residual;
  a.res_q = residual_q;
  a.res_scale = residual_q ? residual_range / 8323072.f : 0.f;
  a.y = y;
  a.y_absmax = y_absmax;
  a.yq = yq;
  a.overflow = overflow;
  a.yq_inv = yq ? 8323072.f / yq_range : 0.f;
  a.inv_qmax = 1.f / 8323072.f;
  a.n = n, a.h = h, a.w = w, a.cin = cin, a.cout = cout;
  a.nfrag = cout / 16, a.relu = relu ? 1 : 0, a.stride = stride, a.pad = pad;
  a.ntw = (a.wo + kNT - 1) / kNT;
  a.tiles_img = ((a.ho + kNT - 1) / kNT) * a.ntw;
  if ((long long)n * a.tiles_img > 0x7fffffffLL) return fail(SMPQ_E_SHAPE, "smpq_conv2d_narrow_fwd_q: too many tiles");
  a.tiles = n * a.tiles_img;
  const bool lean = yq && !y && !y_absmax && !residual;
  hipStream_t s = (hipStream_t)stream;
  if (wlimbs == 3) return launch_narrow_w<3, false>(a, lean, s);
  return a.w_off ? launch_narrow_w<1, true>(a, lean, s) : launch_narrow_w<1, false>(a, lean, s);
}
