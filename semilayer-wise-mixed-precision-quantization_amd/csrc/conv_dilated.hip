// Dilated 3x3 quantized conv (stride 1, padding = dilation = d in {2, 4, 8}, groups 1) for gfx950 on
// v_mfma_i32_16x16x64_i8: the conv2 of a Bottleneck built with replace_stride_with_dilation
// (resnet.py conv3x3 with dilation > 1), eval BatchNorm and ReLU folded in, on 3 activation limbs and
// 1 or 3 weight limbs.
//
// Phase rule. Write an output pixel as oh = ph + d i, ow = pw + d j (0 <= ph, pw < d). Tap (kr, kc)
// reads input (oh + (kr - 1) d, ow + (kc - 1) d) = lattice pixel (i + kr - 1, j + kc - 1) of the SAME
// phase, zero outside 0 <= i' < LH(ph) = ceil((h - ph) / d), 0 <= j' < LW(pw) = ceil((w - pw) / d).
// So the conv is d * d independent 3x3 / pad 1 convs, one per phase lattice, and a (T + 2) x (T + 2)
// halo patch of LATTICE pixels staged once serves all nine taps, as in conv_halo.hip for d = 1: the
// staged bytes per output do not grow with d.
//
// Work split. A workgroup of 4 waves owns one image, one phase, one 8 x 8 tile of that phase's
// lattice and 64 output channels; wave v owns lattice rows 2 v, 2 v + 1 of the tile (one 16-pixel MFMA
// fragment) and all 64 channels (four A fragments per tap and weight limb). The grid is sized by the
// largest lattice (phase 0); a tile outside its own phase's lattice (smaller extents when d does not
// divide h or w, none at all when ph >= h) returns before any DMA or barrier. Tiles are ordered as
// the halo kernel orders them: the channel tiles of one patch adjacent, then neighbouring patches,
// with the same XCD remap.
//
// Per 64-channel input chunk the workgroup stages by LDS-DMA (lds_dma.h dma16)
//   * the 10 x 10 lattice patch of the three activation limbs: per-lane sources step d * cin along a
//     lattice row and d * w * cin between rows; a lattice position outside the image gets the
//     out-of-range buffer offset, which the DMA stages as zero;
//   * the chunk's weights of all nine taps and LW weight limbs, from the dense pack
//     ([LW][cout][9 cin] or its K-major copy [LW][9 cin / 64][cout][64], ConvArgs-style w_kmajor).
// LDS images are the halo kernel's: patch [limb][pr][pc][64] with 16-B chunk c at c ^ 2 (pr & 1),
// weights [limb][tap][64 couts][64] with swz<64>; fragment reads are conflict-free for the same
// reason (tools/halo_conflicts.py) and tap offsets are compile-time. One stage: refilled after a
// barrier per chunk. LDS = LW * 36 KiB + 19 KiB.
//
// Weight offsets (one weight limb: weight = code + offset[c]): the correction is offset[c] times the
// digit sum of the staged window; out-of-lattice taps were staged as zero, so the sum runs over the
// in-range taps only.
//
// Epilogues: conv_common.h / lds_dma.h arithmetic (limb_smin / limb_nacc passes, lean_v1, affine,
// lean_quad, encode4), so a value is rounded as the dense kernels round it: the lean static-range form
// when only limb planes are wanted, the general form (fp32 y, y_absmax, limb planes) otherwise. No
// residual. Output stores go to lattice pixels (pitch d * cout): after the lane-group transpose a
// pixel's 64 channels of one limb plane are 4 x 16 B = one half cache line. Every global access of a
// tensor goes through a range-checked buffer resource with 32-bit offsets.
#include "lds_dma.h"

namespace smpq {
namespace {

constexpr int kDT = 8;                                                    // lattice tile edge
constexpr int kDWaves = 4;
constexpr int kDP = kDT + 2;                                              // patch edge
constexpr int kDWB = 9 * 64 * 64;                                         // one weight limb: [tap][64 couts][64 B]
constexpr int kDPB = (3 * kDP * kDP * 64 + 1023) / 1024 * 1024;           // patch image in whole DMA pieces
constexpr long long kDBytesMax = 0x7fffff00LL;

struct DilatedArgs {
  const int8_t* xq;       // [3][n][h][w][cin]
  long long plane;        // bytes per activation limb plane
  const float* x_absmax;  // [n]
  const int8_t* codes;    // [LW][cout][9 cin], or K-major [LW][9 cin / 64][cout][64]
  long long wplane;       // bytes per weight limb plane
  const int32_t* w_off;   // [cout] or NULL
  const float* col_scale;
  const float* col_shift;
  float* y;
  float* y_absmax;
  int8_t* yq;
  int32_t* overflow;
  float yq_inv, inv_qmax;
  int n, h, w, cin, cout, d, relu, w_kmajor;
  int nct, ntw, ntile, tiles_img;  // channel tiles; column tiles, tiles of one phase, tiles of one image
};

// LW weight limbs (1 or 3), OFF: weight offsets (LW == 1), LEAN: the static-range limb-plane epilogue
template <int LW, bool OFF, bool LEAN>
__global__ __launch_bounds__(64 * kDWaves) void qconv_dilated_kernel(DilatedArgs a) {
  constexpr int L = 3;
  constexpr int SMIN = limb_smin(L, LW), NACC = limb_nacc(L, LW);
  constexpr int PW = kDP, NPX = kDP * kDP, PLIMB = NPX * 64;
  constexpr int WB = LW * kDWB;
  constexpr int PPIECE = kDPB / 1024;
  constexpr int PSL = (PPIECE + kDWaves - 1) / kDWaves;
  static_assert(!OFF || LW == 1, "weight offsets come with one weight limb");
  extern __shared__ __attribute__((aligned(1024))) int8_t lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __builtin_assume(wave >= 0 && wave < kDWaves);
  const int frow = lane & 15, grp = lane >> 4;

  // ---- tile: the halo kernel's XCD-aware order ----------------------------------------------------
  const int total = gridDim.x, full = total & ~7;
  int t = blockIdx.x;
  if (t < full) t = (t & 7) * (full >> 3) + (t >> 3);
  const int ct = t % a.nct, s = t / a.nct;
  const int img = s / a.tiles_img, rem = s - img * a.tiles_img;
  const int phase = rem / a.ntile, tl = rem - phase * a.ntile;
  const int ph = phase / a.d, pw = phase - ph * a.d;
  const int tr = tl / a.ntw, tc = tl - tr * a.ntw;
  const int i0 = tr * kDT, j0 = tc * kDT;
  // this phase's lattice (0 when the phase has no pixel: ph >= h)
  const int lh = (a.h - ph + a.d - 1) / a.d, lw = (a.w - pw + a.d - 1) / a.d;
  if (i0 >= lh || j0 >= lw) return;  // (workgroup-uniform, before any DMA or barrier)
  const int nch = a.cin / 64;

  const v4i wrs = make_rsrc(a.codes, (long long)LW * a.wplane);
  const v4i xrs = make_rsrc(a.xq, (long long)L * a.plane);

  // ---- per-lane DMA sources (fixed over the chunks; limb, tap and chunk move the scalar offset) ----
  // weight piece (limb, tap, wave): couts 16 wave .. + 15 of this channel tile, 4 lanes per cout row;
  // patch piece q = wave + 4 k (< PPIECE): LDS bytes [1024 q, + 1024) of the [L][10][10][64] image,
  // i.e. patch pixels 16 q .. 16 q + 15 (4 lanes per pixel)
  unsigned wsrc, psrc[PSL];
  {
    const int row = lane >> 2;
    const int lc = (lane & 3) ^ swz<64>(row);
    const int cr = ct * 64 + 16 * wave + row;
    wsrc = a.w_kmajor ? (unsigned)(cr * 64 + 16 * lc) : (unsigned)(cr * 9 * a.cin + 16 * lc);
  }
  const unsigned tapstride = __builtin_amdgcn_readfirstlane(a.w_kmajor ? (unsigned)(nch * a.cout * 64) : (unsigned)a.cin);
  const unsigned wchunk = __builtin_amdgcn_readfirstlane(a.w_kmajor ? (unsigned)(a.cout * 64) : 64u);
#pragma unroll
  for (int k = 0; k < PSL; ++k) {
    const int q = wave + kDWaves * k;
    const int P = 16 * q + (lane >> 2);
    const int l = P / NPX, rp = P - l * NPX;
    const int pr = rp / PW, pc = rp - pr * PW;
    const int li = i0 - 1 + pr, lj = j0 - 1 + pc;  // lattice pixel
    const bool ok = q < PPIECE && l < L && li >= 0 && li < lh && lj >= 0 && lj < lw;
    const int ih = ph + a.d * li, iw = pw + a.d * lj;
    const int c16 = (16 * (lane & 3)) ^ (32 * (pr & 1));
    psrc[k] = ok ? (unsigned)l * (unsigned)a.plane + (unsigned)(((img * a.h + ih) * a.w + iw) * a.cin + c16) : kOOB;
  }
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds));
  auto issue = [&](int cc) {
#pragma unroll
    for (int lw_ = 0; lw_ < LW; ++lw_)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        dma16(lds0 + (unsigned)(lw_ * kDWB + (4 * tap + wave) * 1024), wrs, wsrc,
              __builtin_amdgcn_readfirstlane((unsigned)lw_ * (unsigned)a.wplane + (unsigned)tap * tapstride +
                                             (unsigned)cc * wchunk));
#pragma unroll
    for (int k = 0; k < PSL; ++k)
      if (wave + kDWaves * k < PPIECE)
        dma16(lds0 + (unsigned)(WB + (wave + kDWaves * k) * 1024), xrs, psrc[k],
              __builtin_amdgcn_readfirstlane((unsigned)cc * 64u));
  };

  // ---- per-lane fragment bases: A + limb * kDWB + tap * 4096 + i * 1024; B + limb * PLIMB + tap -----
  const int wrd = frow * 64 + 16 * (grp ^ swz<64>(frow));
  const int r = 2 * wave + (frow >> 3), c = frow & 7;  // this lane's tile pixel
  int bpar[2];                                         // [1] for odd kr (the row parity flips the XOR)
#pragma unroll
  for (int par = 0; par < 2; ++par) bpar[par] = WB + (r * PW + c) * 64 + 16 * (grp ^ (2 * ((r + par) & 1)));

  v4i acc[NACC][4];
#pragma unroll
  for (int s_ = 0; s_ < NACC; ++s_)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[s_][i] = v4i{0, 0, 0, 0};
  int rs[L] = {0, 0, 0};  // OFF: this lane's share of the window digit sums

  for (int cc = 0; cc < nch; ++cc) {
    if (cc) {  // every wave is done with the last chunk
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    issue(cc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int kr = 0; kr < 3; ++kr)
#pragma unroll
      for (int kc = 0; kc < 3; ++kc) {
        const int tap = kr * 3 + kc;
        v4i fa[LW][4], fb[L];
#pragma unroll
        for (int lw_ = 0; lw_ < LW; ++lw_)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            fa[lw_][i] = *reinterpret_cast<const v4i*>(lds + lw_ * kDWB + wrd + tap * 4096 + i * 1024);
#pragma unroll
        for (int l = 0; l < L; ++l)
          fb[l] = *reinterpret_cast<const v4i*>(lds + bpar[kr & 1] + l * PLIMB + (kr * PW + kc) * 64);
        if constexpr (OFF) {
#pragma unroll
          for (int l = 0; l < L; ++l) {
            int sacc = rs[l];
            sacc = __builtin_amdgcn_sdot4(fb[l].x, 0x01010101, sacc, false);
            sacc = __builtin_amdgcn_sdot4(fb[l].y, 0x01010101, sacc, false);
            sacc = __builtin_amdgcn_sdot4(fb[l].z, 0x01010101, sacc, false);
            sacc = __builtin_amdgcn_sdot4(fb[l].w, 0x01010101, sacc, false);
            rs[l] = sacc;
          }
        }
#pragma unroll
        for (int la = 0; la < L; ++la)
#pragma unroll
          for (int lw_ = 0; lw_ < LW; ++lw_)
            if (la + lw_ >= SMIN) {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                acc[la + lw_ - SMIN][i] =
                    __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[lw_][i], fb[la], acc[la + lw_ - SMIN][i], 0, 0, 0);
            }
      }
  }

  // ---- epilogue: lane = channels ct * 64 + 16 i + 4 grp .. + 3 of tile pixel (r, c) -----------------
  if constexpr (OFF) {  // weight = code + offset: + offset[c] * (window digit sum, all 64 * nch * 9 K)
#pragma unroll
    for (int l = 0; l < L; ++l) {
      int sacc = rs[l];
      sacc += __shfl_xor(sacc, 16, kWave);
      sacc += __shfl_xor(sacc, 32, kWave);
      rs[l] = sacc;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int4 coff = *reinterpret_cast<const int4*>(a.w_off + ct * 64 + 16 * i + 4 * grp);
      const int cor[4] = {coff.x, coff.y, coff.z, coff.w};
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[l][i][e] += cor[e] * rs[l];
    }
  }
  const bool ok = i0 + r < lh && j0 + c < lw;
  const int oh = ph + a.d * (i0 + r), ow = pw + a.d * (j0 + c);
  const long long oplane = (long long)a.n * a.h * a.w * a.cout;  // elements per output plane
  const unsigned eo = ok ? (unsigned)(((img * a.h + oh) * a.w + ow) * a.cout + ct * 64) : 0u;
  const auto yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y ? (int)(4 * oplane) : 0, 0x00020000);
  const auto qrs = __builtin_amdgcn_make_buffer_rsrc(a.yq, 0, a.yq ? (int)(L * oplane) : 0, 0x00020000);
  constexpr float qmax = act_qmax<L>();
  const bool relu = a.relu != 0;
  const float rscale = a.x_absmax[img] * a.inv_qmax;
  const float inv = a.yq_inv;
  unsigned wq[4][L];
  float vmax = 0.f;  // LEAN: the largest rounded code; otherwise max |y|
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c4 = ct * 64 + 16 * i + 4 * grp;
    const float4 cs = *reinterpret_cast<const float4*>(a.col_scale + c4);
    const float4 csh = *reinterpret_cast<const float4*>(a.col_shift + c4);
    v4i accq[NACC];
#pragma unroll
    for (int s_ = 0; s_ < NACC; ++s_) accq[s_] = acc[s_][i];
    if constexpr (LEAN) {
      const float csq[4] = {cs.x * inv, cs.y * inv, cs.z * inv, cs.w * inv};
      const float shq[4] = {csh.x * inv, csh.y * inv, csh.z * inv, csh.w * inv};
      const int none[4] = {0, 0, 0, 0};
      const float m = lean_quad<L, NACC, SMIN>(accq, rscale, csq, shq, false, none, 0.f, relu, relu ? 0.f : -qmax, wq[i]);
      vmax = ok ? fmaxf(vmax, m) : vmax;
    } else {
      const float csr[4] = {cs.x, cs.y, cs.z, cs.w}, shr[4] = {csh.x, csh.y, csh.z, csh.w};
      float o[4];
      float am = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = affine(lean_v1<NACC, SMIN>(accq, e), rscale, csr[e], shr[e]);
        if (relu) o[e] = fmaxf(o[e], 0.f);
        am = fmaxf(am, fabsf(o[e]));
      }
      if (ok) vmax = fmaxf(vmax, am);
      if (a.y) {
        const v4u v = {__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])};
        __builtin_amdgcn_raw_buffer_store_b128(v, yrs, ok ? 4u * (eo + 16u * (unsigned)i + 4u * (unsigned)grp) : kOOB, 0, 0);
      }
      if (a.yq) {
        int q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = (int)fminf(fmaxf(rintf(__fmul_rn(o[e], inv)), -qmax), qmax);
        encode4<L>(q, wq[i]);
      }
    }
  }
  if constexpr (!LEAN) {
    if (a.y_absmax) {
      const float m = wave_max(vmax);
      if (lane == 0 && m > 0.f) atomic_max_nonneg(&a.y_absmax[img], m);
    }
  }
  if (a.yq) {
    // after the transpose lane group g holds the 16 channels of block g of its pixel: one 16-B store per
    // limb plane, the four groups of a pixel filling 64 contiguous bytes
#pragma unroll
    for (int l = 0; l < L; ++l) {
      unsigned w0 = wq[0][l], w1 = wq[1][l], w2 = wq[2][l], w3 = wq[3][l];
      transpose4(w0, w1, w2, w3);
      __builtin_amdgcn_raw_buffer_store_b128(v4u{w0, w1, w2, w3}, qrs,
                                             ok ? eo + 16u * (unsigned)grp + (unsigned)(l * oplane) : kOOB, 0, 0);
    }
    const bool ovf = LEAN ? vmax > qmax : rintf(__fmul_rn(vmax, a.yq_inv)) > qmax;
    if (__any(ovf) && lane == 0) atomicMax(a.overflow, 1);
  }
}

template <int LW, bool OFF, bool LEAN>
int launch_dilated_one(const DilatedArgs& a, unsigned blocks, hipStream_t stream) {
  constexpr int lds_bytes = LW * kDWB + kDPB;
  static_assert(lds_bytes <= 160 * 1024, "LDS per workgroup on gfx950");
  const auto fn = qconv_dilated_kernel<LW, OFF, LEAN>;
  static const hipError_t attr = [&] {
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  }();
  if (attr != hipSuccess) return check_hip(attr, "qconv_dilated_kernel LDS attribute");
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * kDWaves), lds_bytes, stream, a);
  return check_hip(hipGetLastError(), "qconv_dilated_kernel launch");
}

bool dilated_supported(int cin, int cout, int kh, int kw, int stride, int pad, int dilation, int limbs, int wlimbs) {
  return kh == 3 && kw == 3 && stride == 1 && pad == dilation && (dilation == 2 || dilation == 4 || dilation == 8) &&
         cin > 0 && cout > 0 && cin % 64 == 0 && cout % 64 == 0 && limbs == 3 && (wlimbs == 1 || wlimbs == 3);
}

}  // namespace
}  // namespace smpq

using namespace smpq;

extern "C" int smpq_conv2d_dilated_supported(int cin, int cout, int kh, int kw, int stride, int pad, int dilation,
                                             int limbs, int wlimbs) {
  return dilated_supported(cin, cout, kh, kw, stride, pad, dilation, limbs, wlimbs) ? 1 : 0;
}

extern "C" int smpq_conv2d_dilated_fwd_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                         const int8_t* codes, const int8_t* codes_kmajor, int wlimbs,
                                         const int32_t* offset, int cout, int kh, int kw, int stride, int pad,
                                         int dilation, const float* col_scale, const float* col_shift, int relu,
                                         int limbs, float* y, float* y_absmax, int8_t* yq, float yq_range,
                                         int32_t* overflow, smpq_stream_t stream) {
  if (!xq || !x_absmax || !codes || !col_scale || !col_shift || (!y && !yq))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_dilated_fwd_q: null pointer");
  if (yq && (!overflow || !(yq_range > 0.f)))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_dilated_fwd_q: yq needs overflow flag and a positive range");
  if (limbs != 3 || (wlimbs != 1 && wlimbs != 3))
    return fail(SMPQ_E_INVALID, "smpq_conv2d_dilated_fwd_q: built for 3 activation limbs and 1 or 3 weight limbs");
  if (n <= 0 || h <= 0 || w <= 0) return fail(SMPQ_E_SHAPE, "smpq_conv2d_dilated_fwd_q: bad shape");
  if (!dilated_supported(cin, cout, kh, kw, stride, pad, dilation, limbs, wlimbs))
    return fail(SMPQ_E_SHAPE, "smpq_conv2d_dilated_fwd_q: unsupported geometry (smpq_conv2d_dilated_supported: 3x3 / "
                              "stride 1 / pad == dilation in {2, 4, 8}, cin % 64 == 0, cout % 64 == 0)");
  if ((((uintptr_t)xq | (uintptr_t)codes | (uintptr_t)codes_kmajor | (uintptr_t)col_scale | (uintptr_t)col_shift |
        (uintptr_t)offset | (uintptr_t)y | (uintptr_t)yq) & 15) != 0)
    return fail(SMPQ_E_INVALID, "smpq_conv2d_dilated_fwd_q: operands must be 16-B aligned");
  DilatedArgs a = {};
  a.plane = (long long)n * h * w * cin;
  const long long oplane = (long long)n * h * w * cout;  // stride 1, pad == dilation: ho = h, wo = w
  // 32-bit buffer offsets over all three limb planes (and the fp32 output): the caller splits the batch
  if (3 * a.plane > kDBytesMax || (yq && 3 * oplane > kDBytesMax) || (y && 4 * oplane > kDBytesMax))
    return fail(SMPQ_E_SHAPE, "smpq_conv2d_dilated_fwd_q: a tensor of 2 GiB or more (split the batch)");
  a.xq = xq;
  a.x_absmax = x_absmax;
  a.codes = codes_kmajor ? codes_kmajor : codes;
  a.w_kmajor = codes_kmajor ? 1 : 0;
  a.wplane = (long long)cout * 9 * cin;
  a.w_off = wlimbs == 1 ? offset : nullptr;
  a.col_scale = col_scale;
  a.col_shift = col_shift;
  a.y = y;
  a.y_absmax = y_absmax;
  a.yq = yq;
  a.overflow = overflow;
  a.yq_inv = yq ? 8323072.f / yq_range : 0.f;
  a.inv_qmax = 1.f / 8323072.f;
  a.n = n, a.h = h, a.w = w, a.cin = cin, a.cout = cout, a.d = dilation, a.relu = relu ? 1 : 0;
  // the grid covers the largest lattice (phase 0) for every phase
  const int lh = (h + dilation - 1) / dilation, lw = (w + dilation - 1) / dilation;
  a.nct = cout / 64;
  a.ntw = (lw + kDT - 1) / kDT;
  a.ntile = ((lh + kDT - 1) / kDT) * a.ntw;
  a.tiles_img = dilation * dilation * a.ntile;
  const long long blocks = (long long)n * a.tiles_img * a.nct;
  if (blocks > 0x7fffffffLL) return fail(SMPQ_E_SHAPE, "smpq_conv2d_dilated_fwd_q: grid too large");
  const bool lean = yq && !y && !y_absmax;
  hipStream_t s = (hipStream_t)stream;
  if (wlimbs == 3)
    return lean ? launch_dilated_one<3, false, true>(a, (unsigned)blocks, s)
                : launch_dilated_one<3, false, false>(a, (unsigned)blocks, s);
  if (a.w_off)
    return lean ? launch_dilated_one<1, true, true>(a, (unsigned)blocks, s)
                : launch_dilated_one<1, true, false>(a, (unsigned)blocks, s);
  return lean ? launch_dilated_one<1, false, true>(a, (unsigned)blocks, s)
              : launch_dilated_one<1, false, false>(a, (unsigned)blocks, s);
}
