// Host twins of the trial row patch (include/smpq.h, "trial row patch"): native C++, no HIP, so a
// stand-alone host program (tools/trial_row_sanitize.cpp) can compile them under a sanitizer.
// quant.hip wraps them as smpq_trial_row_patch_host / smpq_trial_row_restore_host and, for n rows of
// one operand (tools/trial_rows_sanitize.cpp), smpq_trial_rows_patch_host / _restore_host. The arithmetic
// restates quantize_row_host and pack_weights_ex_kernel (lw >= 2) of quant.hip; FP contraction off.
// At the end: the twins of the trial rows conv (trial_conv.hip wraps them).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smpq.h"

#pragma clang fp contract(off)

namespace smpq {

// Argument checks shared by the device and host entry points (km may be null); "" when they pass.
inline int trial_row_check(const void* w, int cout, int cin, int kh, int kw, int channel, int bits, int semantics,
                           int wlimbs, const void* bn_a, const void* codes, const void* wscale,
                           const void* col_scale, const void* save, const void* status, std::string* err,
                           const char* fn = "smpq_trial_row_patch") {
  const std::string who(fn);
  if (!w || !bn_a || !codes || !wscale || !col_scale || !save || !status) {
    *err = who + ": null pointer";
    return SMPQ_E_INVALID;
  }
  if (cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) {
    *err = who + ": sizes must be positive";
    return SMPQ_E_INVALID;
  }
  if (wlimbs < 2 || wlimbs > 3) {
    *err = who + ": wlimbs must be 2 or 3";
    return SMPQ_E_INVALID;
  }
  if (channel < 0 || channel >= cout) {
    *err = who + ": channel outside [0, cout)";
    return SMPQ_E_INVALID;
  }
  if (semantics != SMPQ_QSEM_CPU && semantics != SMPQ_QSEM_DEVICE) {
    *err = who + ": semantics must be SMPQ_QSEM_CPU or SMPQ_QSEM_DEVICE";
    return SMPQ_E_INVALID;
  }
  if ((uintptr_t)save & 3) {
    *err = who + ": save area must be 4-byte aligned";
    return SMPQ_E_INVALID;
  }
  if (cin % 64 != 0 || (long long)cin * kh * kw > SMPQ_TRIAL_MAX_K) {
    *err = who + ": cin must be a multiple of 64 and K at most SMPQ_TRIAL_MAX_K";
    return SMPQ_E_SHAPE;
  }
  if (bits < 1 || bits > 16) {
    *err = who + ": bits outside 1..16";
    return SMPQ_E_BITS;
  }
  return SMPQ_OK;
}

inline int trial_restore_check(int cout, int K, int channel, int wlimbs, const void* codes, const void* wscale,
                               const void* col_scale, const void* save, std::string* err) {
  if (!codes || !wscale || !col_scale || !save) {
    *err = "smpq_trial_row_restore: null pointer";
    return SMPQ_E_INVALID;
  }
  if (cout <= 0 || K <= 0 || wlimbs < 2 || wlimbs > 3 || channel < 0 || channel >= cout || ((uintptr_t)save & 3)) {
    *err = "smpq_trial_row_restore: need cout, K > 0, wlimbs 2 or 3, channel in [0, cout), an aligned save area";
    return SMPQ_E_INVALID;
  }
  if (K % 64 != 0 || K > SMPQ_TRIAL_MAX_K) {
    *err = "smpq_trial_row_restore: K must be a multiple of 64, at most SMPQ_TRIAL_MAX_K";
    return SMPQ_E_SHAPE;
  }
  return SMPQ_OK;
}

// One row, arguments already checked: save, then steps 1-5 of the header.
inline void trial_row_patch_body_host(const float* w, int cout, int cin, int kh, int kw, int channel, int bits,
                                      int semantics, int wlimbs, const float* bn_a, int8_t* codes, float* wscale,
                                      float* col_scale, void* save, int32_t* status) {
  const int taps = kh * kw, K = cin * taps, c = channel;
  const size_t wplane = (size_t)cout * K;
  const float* row = w + (size_t)c * K;
  float* shead = static_cast<float*>(save);
  int8_t* scodes = static_cast<int8_t*>(save) + SMPQ_TRIAL_SAVE_HEADER;
  shead[0] = wscale[c];
  shead[1] = col_scale[c];
  for (int l = 0; l < wlimbs; ++l) std::memcpy(scodes + (size_t)l * K, codes + l * wplane + (size_t)c * K, K);
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < K; ++i) {
    mn = std::fmin(mn, row[i]);
    mx = std::fmax(mx, row[i]);
  }
  if (mx == mn) {
    *status = 1;
    return;
  }
  // the quantizer (quantize_row_host), into a scratch row
  const double scale = ((double)mx - (double)mn) / (double)((1 << bits) - 1);
  const double zd = std::nearbyint((double)mn / scale) + 0.0;
  const float s = (float)scale;
  const float z32 = (float)zd;
  const float inv32 = (float)(1.0 / scale);
  std::vector<float> q(K);
  for (int i = 0; i < K; ++i) {
    const float d = semantics == SMPQ_QSEM_DEVICE ? row[i] * inv32 : row[i] / s;
    q[i] = (std::nearbyintf(d + z32) - z32) * s;
  }
  // the coder (pack_weights_ex_kernel, lw >= 2) with step s
  const float wmax = wlimbs >= 3 ? 8323072.f : 32512.f;
  int mmin = INT32_MAX, mmax = INT32_MIN;
  bool bad = !(s > 0.f);
  float amax = 0.f;
  for (int i = 0; i < K; ++i) {
    const float v = q[i];
    amax = std::fmax(amax, std::fabs(v));
    if (bad) continue;
    const float mf = std::nearbyintf(v / s);
    if (mf * s != v || std::fabs(mf) > wmax) {
      bad = true;
      continue;
    }
    mmin = mmin < (int)mf ? mmin : (int)mf;
    mmax = mmax > (int)mf ? mmax : (int)mf;
  }
  float sc = s;
  int sh = 0;
  if (bad) {
    sc = amax > 0.f ? amax / wmax : 1.f;
  } else {
    const int am = std::abs(mmin) > std::abs(mmax) ? std::abs(mmin) : std::abs(mmax);
    const int lim = (int)wmax;
    while (am > 0 && sh < 8 * (wlimbs - 1) && (am << (sh + 1)) <= lim) ++sh;
    sc = std::ldexp(s, -sh);
  }
  for (int k = 0; k < K; ++k) {
    const int tap = k / cin, ci = k - tap * cin;
    const float v = q[ci * taps + tap];
    int m;
    if (bad) m = (int)std::fmin(std::fmax(std::nearbyint((double)v / (double)sc), -(double)wmax), (double)wmax);
    else m = (int)std::nearbyintf(v / s) * (1 << sh);
    for (int l = 0; l < wlimbs; ++l) {
      const int lo = (l == wlimbs - 1) ? m : ((m + 128) & 255) - 128;
      codes[l * wplane + (size_t)c * K + k] = (int8_t)lo;
      m = (m - lo) >> 8;
    }
  }
  wscale[c] = sc;
  col_scale[c] = sc * bn_a[c];
}

inline int trial_row_patch_host(const float* w, int cout, int cin, int kh, int kw, int channel, int bits,
                                int semantics, int wlimbs, const float* bn_a, int8_t* codes, float* wscale,
                                float* col_scale, void* save, int32_t* status, std::string* err) {
  const int rc = trial_row_check(w, cout, cin, kh, kw, channel, bits, semantics, wlimbs, bn_a, codes, wscale,
                                 col_scale, save, status, err);
  if (rc != SMPQ_OK) return rc;
  trial_row_patch_body_host(w, cout, cin, kh, kw, channel, bits, semantics, wlimbs, bn_a, codes, wscale, col_scale,
                            save, status);
  return SMPQ_OK;
}

inline int trial_row_restore_host(int cout, int K, int channel, int wlimbs, int8_t* codes, float* wscale,
                                  float* col_scale, const void* save, std::string* err) {
  const int rc = trial_restore_check(cout, K, channel, wlimbs, codes, wscale, col_scale, save, err);
  if (rc != SMPQ_OK) return rc;
  const float* shead = static_cast<const float*>(save);
  const int8_t* scodes = static_cast<const int8_t*>(save) + SMPQ_TRIAL_SAVE_HEADER;
  const size_t wplane = (size_t)cout * K;
  for (int l = 0; l < wlimbs; ++l) std::memcpy(codes + l * wplane + (size_t)channel * K, scodes + (size_t)l * K, K);
  wscale[channel] = shead[0];
  col_scale[channel] = shead[1];
  return SMPQ_OK;
}

// ---- n rows of one operand (include/smpq.h, "trial rows patch") ----------------------------------
// What both rows entry points check without reading the lists (the device one gets device lists).
inline int trial_rows_check(const void* w, int cout, int cin, int kh, int kw, const void* channels, const void* bits,
                            int n, int semantics, int wlimbs, const void* bn_a, const void* codes, const void* wscale,
                            const void* col_scale, const void* save, const void* status, std::string* err) {
  if (!channels || !bits) {
    *err = "smpq_trial_rows_patch: null pointer";
    return SMPQ_E_INVALID;
  }
  const int rc = trial_row_check(w, cout, cin, kh, kw, 0, 8, semantics, wlimbs, bn_a, codes, wscale, col_scale, save,
                                 status, err, "smpq_trial_rows_patch");
  if (rc != SMPQ_OK) return rc;
  if (n < 1 || n > cout) {
    *err = "smpq_trial_rows_patch: n outside 1..cout";
    return SMPQ_E_INVALID;
  }
  return SMPQ_OK;
}

inline int trial_rows_restore_check(int cout, int K, const void* channels, int n, int wlimbs, const void* codes,
                                    const void* wscale, const void* col_scale, const void* save, std::string* err) {
  if (!channels) {
    *err = "smpq_trial_rows_restore: null pointer";
    return SMPQ_E_INVALID;
  }
  const int rc = trial_restore_check(cout, K, 0, wlimbs, codes, wscale, col_scale, save, err);
  if (rc != SMPQ_OK) {
    err->replace(0, std::strlen("smpq_trial_row_restore"), "smpq_trial_rows_restore");
    return rc;
  }
  if (n < 1 || n > cout) {
    *err = "smpq_trial_rows_restore: n outside 1..cout";
    return SMPQ_E_INVALID;
  }
  return SMPQ_OK;
}

// The lists themselves (host memory): every channel in range and seen once, every bit-width in 1..16.
inline int trial_rows_lists_check(const char* fn, int cout, const int32_t* channels, const int32_t* bits, int n,
                                  std::string* err, int maxbits = 16) {
  std::vector<char> seen((size_t)cout, 0);
  for (int i = 0; i < n; ++i) {
    const int c = channels[i];
    if (c < 0 || c >= cout) {
      *err = std::string(fn) + ": channel outside [0, cout)";
      return SMPQ_E_INVALID;
    }
    if (bits && (bits[i] < 1 || bits[i] > maxbits)) {
      *err = std::string(fn) + ": bits outside 1.." + std::to_string(maxbits);
      return SMPQ_E_BITS;
    }
    if (seen[c]) {
      *err = std::string(fn) + ": channel " + std::to_string(c) + " listed twice";
      return SMPQ_E_INVALID;
    }
    seen[c] = 1;
  }
  return SMPQ_OK;
}

inline int trial_rows_patch_host(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                                 const int32_t* bits, int n, int semantics, int wlimbs, const float* bn_a,
                                 int8_t* codes, float* wscale, float* col_scale, void* save, int32_t* status,
                                 std::string* err) {
  int rc = trial_rows_check(w, cout, cin, kh, kw, channels, bits, n, semantics, wlimbs, bn_a, codes, wscale, col_scale,
                            save, status, err);
  if (rc == SMPQ_OK) rc = trial_rows_lists_check("smpq_trial_rows_patch", cout, channels, bits, n, err);
  if (rc != SMPQ_OK) return rc;
  const size_t slot = SMPQ_TRIAL_SAVE_HEADER + (size_t)wlimbs * cin * kh * kw;
  for (int i = 0; i < n; ++i)
    trial_row_patch_body_host(w, cout, cin, kh, kw, channels[i], bits[i], semantics, wlimbs, bn_a, codes, wscale,
                              col_scale, static_cast<int8_t*>(save) + i * slot, status + i);
  return SMPQ_OK;
}

inline int trial_rows_restore_host(int cout, int K, const int32_t* channels, int n, int wlimbs, int8_t* codes,
                                   float* wscale, float* col_scale, const void* save, std::string* err) {
  int rc = trial_rows_restore_check(cout, K, channels, n, wlimbs, codes, wscale, col_scale, save, err);
  if (rc == SMPQ_OK) rc = trial_rows_lists_check("smpq_trial_rows_restore", cout, channels, nullptr, n, err);
  if (rc != SMPQ_OK) return rc;
  const size_t slot = SMPQ_TRIAL_SAVE_HEADER + (size_t)wlimbs * K;
  for (int i = 0; i < n; ++i) {
    rc = trial_row_restore_host(cout, K, channels[i], wlimbs, codes, wscale, col_scale,
                                static_cast<const int8_t*>(save) + i * slot, err);
    if (rc != SMPQ_OK) return rc;
  }
  return SMPQ_OK;
}

// ---- n rows of one exact8 operand (include/smpq.h, "trial rows patch, exact8 operands") -----------
// One int8 plane, a per-channel offset (or none), wscale = the step. The arithmetic restates
// quantize_row_host and pack_weights_ex_kernel (lw == 1) of quant.hip; quant.hip wraps these as
// smpq_trial_rows_patch_x8_host / _restore_x8_host (tools/trial_rows_x8_sanitize.cpp).
inline int trial_rows_x8_check(const char* fn, const void* w, int cout, int cin, int kh, int kw, const void* channels,
                               const void* bits, int n, int semantics, const void* bn_a, const void* codes,
                               const void* wscale, const void* col_scale, const void* save, const void* status,
                               std::string* err) {
  const std::string who(fn);
  if (!w || !channels || !bits || !bn_a || !codes || !wscale || !col_scale || !save || !status) {
    *err = who + ": null pointer";
    return SMPQ_E_INVALID;
  }
  if (cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) {
    *err = who + ": sizes must be positive";
    return SMPQ_E_INVALID;
  }
  if (semantics != SMPQ_QSEM_CPU && semantics != SMPQ_QSEM_DEVICE) {
    *err = who + ": semantics must be SMPQ_QSEM_CPU or SMPQ_QSEM_DEVICE";
    return SMPQ_E_INVALID;
  }
  if ((uintptr_t)save & 3) {
    *err = who + ": save area must be 4-byte aligned";
    return SMPQ_E_INVALID;
  }
  if (n < 1 || n > cout) {
    *err = who + ": n outside 1..cout";
    return SMPQ_E_INVALID;
  }
  if (cin % 64 != 0 || (long long)cin * kh * kw > SMPQ_TRIAL_MAX_K) {
    *err = who + ": cin must be a multiple of 64 and K at most SMPQ_TRIAL_MAX_K";
    return SMPQ_E_SHAPE;
  }
  return SMPQ_OK;
}

inline int trial_rows_restore_x8_check(const char* fn, int cout, int K, const void* channels, int n, const void* codes,
                                       const void* wscale, const void* col_scale, const void* save, std::string* err) {
  const std::string who(fn);
  if (!channels || !codes || !wscale || !col_scale || !save) {
    *err = who + ": null pointer";
    return SMPQ_E_INVALID;
  }
  if (cout <= 0 || K <= 0 || n < 1 || n > cout || ((uintptr_t)save & 3)) {
    *err = who + ": need cout, K > 0, n in 1..cout, an aligned save area";
    return SMPQ_E_INVALID;
  }
  if (K % 64 != 0 || K > SMPQ_TRIAL_MAX_K) {
    *err = who + ": K must be a multiple of 64, at most SMPQ_TRIAL_MAX_K";
    return SMPQ_E_SHAPE;
  }
  return SMPQ_OK;
}

// One row, arguments already checked: save, then the header's steps; a nonzero status leaves the
// operand as it is.
inline void trial_row_patch_x8_body_host(const float* w, int cin, int kh, int kw, int c, int bits, int semantics,
                                         const float* bn_a, int8_t* codes, int32_t* offset, float* wscale,
                                         float* col_scale, void* save, int32_t* status) {
  const int taps = kh * kw, K = cin * taps;
  const float* row = w + (size_t)c * K;
  float* shead = static_cast<float*>(save);
  int8_t* scodes = static_cast<int8_t*>(save) + SMPQ_TRIAL_SAVE_HEADER;
  shead[0] = wscale[c];
  shead[1] = col_scale[c];
  const int32_t o_old = offset ? offset[c] : 0;
  std::memcpy(static_cast<int8_t*>(save) + 8, &o_old, sizeof o_old);
  std::memcpy(scodes, codes + (size_t)c * K, K);
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < K; ++i) {
    mn = std::fmin(mn, row[i]);
    mx = std::fmax(mx, row[i]);
  }
  if (mx == mn) {
    *status = 1;
    return;
  }
  const double scale = ((double)mx - (double)mn) / (double)((1 << bits) - 1);
  const double zd = std::nearbyint((double)mn / scale) + 0.0;
  const float s = (float)scale;
  const float z32 = (float)zd;
  const float inv32 = (float)(1.0 / scale);
  std::vector<int> m(K);
  int mmin = INT32_MAX, mmax = INT32_MIN;
  bool bad = !(s > 0.f);
  for (int i = 0; i < K && !bad; ++i) {
    const float d = semantics == SMPQ_QSEM_DEVICE ? row[i] * inv32 : row[i] / s;
    const float v = (std::nearbyintf(d + z32) - z32) * s;
    const float mf = std::nearbyintf(v / s);
    if (mf * s != v || std::fabs(mf) > 32512.f) {
      bad = true;
      break;
    }
    m[i] = (int)mf;
    mmin = mmin < m[i] ? mmin : m[i];
    mmax = mmax > m[i] ? mmax : m[i];
  }
  if (bad || mmax - mmin > 255) {
    *status = 3;
    return;
  }
  const int o = (mmin < -128 || mmax > 127) ? mmin + 128 : 0;
  if (o != 0 && !offset) {
    *status = 4;
    return;
  }
  for (int k = 0; k < K; ++k) {
    const int tap = k / cin, ci = k - tap * cin;
    codes[(size_t)c * K + k] = (int8_t)(m[ci * taps + tap] - o);
  }
  if (offset) offset[c] = o;
  wscale[c] = s;
  col_scale[c] = s * bn_a[c];
}

inline int trial_rows_patch_x8_host(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                                    const int32_t* bits, int n, int semantics, const float* bn_a, int8_t* codes,
                                    int32_t* offset, float* wscale, float* col_scale, void* save, int32_t* status,
                                    std::string* err) {
  const char* fn = "smpq_trial_rows_patch_x8";
  int rc = trial_rows_x8_check(fn, w, cout, cin, kh, kw, channels, bits, n, semantics, bn_a, codes, wscale, col_scale,
                               save, status, err);
  if (rc == SMPQ_OK) rc = trial_rows_lists_check(fn, cout, channels, bits, n, err, 8);
  if (rc != SMPQ_OK) return rc;
  const size_t slot = SMPQ_TRIAL_SAVE_HEADER + (size_t)cin * kh * kw;
  for (int i = 0; i < n; ++i)
    trial_row_patch_x8_body_host(w, cin, kh, kw, channels[i], bits[i], semantics, bn_a, codes, offset, wscale,
                                 col_scale, static_cast<int8_t*>(save) + i * slot, status + i);
  return SMPQ_OK;
}

inline int trial_rows_restore_x8_host(int cout, int K, const int32_t* channels, int n, int8_t* codes, int32_t* offset,
                                      float* wscale, float* col_scale, const void* save, std::string* err) {
  const char* fn = "smpq_trial_rows_restore_x8";
  int rc = trial_rows_restore_x8_check(fn, cout, K, channels, n, codes, wscale, col_scale, save, err);
  if (rc == SMPQ_OK) rc = trial_rows_lists_check(fn, cout, channels, nullptr, n, err);
  if (rc != SMPQ_OK) return rc;
  const size_t slot = SMPQ_TRIAL_SAVE_HEADER + (size_t)K;
  for (int i = 0; i < n; ++i) {
    const int8_t* s = static_cast<const int8_t*>(save) + i * slot;
    const int c = channels[i];
    std::memcpy(codes + (size_t)c * K, s + SMPQ_TRIAL_SAVE_HEADER, K);
    if (offset) std::memcpy(offset + c, s + 8, sizeof(int32_t));
    wscale[c] = reinterpret_cast<const float*>(s)[0];
    col_scale[c] = reinterpret_cast<const float*>(s)[1];
  }
  return SMPQ_OK;
}

// ---- trial rows conv: listed output channels of one conv into held limb planes ---------------------
// (include/smpq.h, "trial rows conv"). quant.hip's neighbour trial_conv.hip wraps the twins as
// smpq_trial_rows_conv_q_host / _restore_host (tools/trial_rows_conv_sanitize.cpp). The arithmetic
// restates lean_v1 / lean_zr / lean_clamp of lds_dma.h with <cmath>; FP contraction off.
inline int trial_rows_conv_check(const char* fn, const void* xq, const void* x_absmax, int n, int h, int w, int cin,
                                 const void* codes, int wlimbs, int cout, int kh, int kw, int stride, int pad,
                                 const void* col_scale, const void* col_shift, int limbs, const void* residual_q,
                                 float residual_range, const void* channels, int nrows, const void* yq,
                                 float yq_range, const void* overflow, const void* save, std::string* err) {
  const std::string who(fn);
  if (!xq || !x_absmax || !codes || !col_scale || !col_shift || !channels || !yq || !overflow || !save) {
    *err = who + ": null pointer";
    return SMPQ_E_INVALID;
  }
  if (limbs < 2 || limbs > 3 || wlimbs < 2 || wlimbs > 3 || (wlimbs == 3 && limbs != 3)) {
    *err = who + ": limbs and wlimbs must be 2 or 3 (3 weight limbs with 3 activation limbs only)";
    return SMPQ_E_INVALID;
  }
  if (!(yq_range > 0.f) || (residual_q && !(residual_range > 0.f))) {
    *err = who + ": ranges must be > 0";
    return SMPQ_E_INVALID;
  }
  if (((uintptr_t)xq | (uintptr_t)codes) & 15) {
    *err = who + ": xq and codes must be 16-byte aligned";
    return SMPQ_E_INVALID;
  }
  if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) {
    *err = who + ": sizes must be positive";
    return SMPQ_E_SHAPE;
  }
  if (nrows < 1 || nrows > cout) {
    *err = who + ": nrows outside 1..cout";
    return SMPQ_E_INVALID;
  }
  const bool k1 = kh == 1 && kw == 1 && stride == 1 && pad == 0, k3 = kh == 3 && kw == 3 && stride == 1 && pad == 1;
  if (!k1 && !k3) {
    *err = who + ": only 1x1 / stride 1 / pad 0 and 3x3 / stride 1 / pad 1";
    return SMPQ_E_SHAPE;
  }
  if (cin % 64 != 0 || (long long)cin * kh * kw > SMPQ_TRIAL_MAX_K || cout % 16 != 0) {
    *err = who + ": cin must be a multiple of 64, K at most SMPQ_TRIAL_MAX_K, cout a multiple of 16";
    return SMPQ_E_SHAPE;
  }
  if ((long long)n * h * w > 0x7fffffffLL) {
    *err = who + ": more than 2^31 - 1 pixels";
    return SMPQ_E_SHAPE;
  }
  return SMPQ_OK;
}

inline int trial_rows_conv_restore_check(const char* fn, const void* channels, int nrows, int limbs, long long pixels,
                                         int cout, const void* yq, const void* save, std::string* err) {
  const std::string who(fn);
  if (!channels || !yq || !save) {
    *err = who + ": null pointer";
    return SMPQ_E_INVALID;
  }
  if (limbs < 2 || limbs > 3 || cout <= 0 || nrows < 1 || nrows > cout) {
    *err = who + ": need limbs 2 or 3, cout > 0, nrows in 1..cout";
    return SMPQ_E_INVALID;
  }
  if (pixels <= 0 || pixels > 0x7fffffffLL) {
    *err = who + ": pixels outside 1..2^31 - 1";
    return SMPQ_E_SHAPE;
  }
  return SMPQ_OK;
}

inline int trial_rows_conv_host(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                const int8_t* codes, int wlimbs, int cout, int kh, int kw, int stride, int pad,
                                const float* col_scale, const float* col_shift, int limbs, const int8_t* residual_q,
                                float residual_range, const int32_t* channels, int nrows, int8_t* yq, float yq_range,
                                int32_t* overflow, void* save, std::string* err) {
  const char* fn = "smpq_trial_rows_conv_q";
  int rc = trial_rows_conv_check(fn, xq, x_absmax, n, h, w, cin, codes, wlimbs, cout, kh, kw, stride, pad, col_scale,
                                 col_shift, limbs, residual_q, residual_range, channels, nrows, yq, yq_range, overflow,
                                 save, err);
  if (rc == SMPQ_OK) rc = trial_rows_lists_check(fn, cout, channels, nullptr, nrows, err);
  if (rc != SMPQ_OK) return rc;
  const int K = cin * kh * kw, L = limbs, LW = wlimbs;
  const int smin = (L + LW - 4) > 0 ? (L + LW - 4) : 0, nacc = L + LW - 1 - smin;
  const long long M = (long long)n * h * w, plane = M * cin, oplane = M * cout, wplane = (long long)cout * K;
  const float qmax = L == 2 ? 32512.f : 8323072.f;
  const float inv = qmax / yq_range, inv_qmax = 1.f / qmax;
  const float rsq = residual_q ? (residual_range / qmax) * inv : 0.f;
  const float w0 = smin == 0 ? 1.f : (smin == 1 ? 256.f : 65536.f);
  int8_t* sv = static_cast<int8_t*>(save);
  for (int i = 0; i < nrows; ++i) {
    const int c = channels[i];
    const float csq = col_scale[c] * inv, shq = col_shift[c] * inv;
    for (long long m = 0; m < M; ++m) {
      const int g = (int)(m / ((long long)h * w)), rem = (int)(m - (long long)g * h * w), oy = rem / w, ox = rem - oy * w;
      int32_t acc[3] = {0, 0, 0};
      for (int tap = 0; tap < kh * kw; ++tap) {
        const int iy = oy + tap / kw - pad, ix = ox + tap % kw - pad;
        if (iy < 0 || iy >= h || ix < 0 || ix >= w) continue;
        const long long src = (((long long)g * h + iy) * w + ix) * cin;
        for (int la = 0; la < L; ++la)
          for (int lw = 0; lw < LW; ++lw) {
            if (la + lw < smin) continue;
            const int8_t* xp = xq + la * plane + src;
            const int8_t* wp = codes + lw * wplane + (long long)c * K + (long long)tap * cin;
            int32_t s = 0;
            for (int k = 0; k < cin; ++k) s += (int32_t)xp[k] * (int32_t)wp[k];
            acc[la + lw - smin] += s;
          }
      }
      float v = (float)acc[0];
      if (smin != 0) v = v * w0;
      for (int t = 1; t < nacc; ++t) v = std::fmaf((float)acc[t], w0 * (float)(1 << (8 * t)), v);
      float z = std::fmaf(v, (x_absmax[g] * inv_qmax) * csq, shq);
      if (residual_q) {
        int32_t r = 0;
        for (int l = L - 1; l >= 0; --l) r = r * 256 + (int32_t)residual_q[l * oplane + m * cout + c];
        z = std::fmaf((float)r, rsq, z);
      }
      const float zr = std::nearbyintf(z);
      if (zr > qmax) *overflow = 1;
      int q = (int)std::fmin(std::fmax(zr, 0.f), qmax);
      for (int l = 0; l < L; ++l) {
        const int lo = (l == L - 1) ? q : ((q + 128) & 255) - 128;
        int8_t* dst = yq + l * oplane + m * cout + c;
        sv[((long long)i * L + l) * M + m] = *dst;
        *dst = (int8_t)lo;
        q = (q - lo) >> 8;
      }
    }
  }
  return SMPQ_OK;
}

inline int trial_rows_conv_restore_host(const int32_t* channels, int nrows, int limbs, long long pixels, int cout,
                                        int8_t* yq, const void* save, std::string* err) {
  const char* fn = "smpq_trial_rows_conv_restore";
  int rc = trial_rows_conv_restore_check(fn, channels, nrows, limbs, pixels, cout, yq, save, err);
  if (rc == SMPQ_OK) rc = trial_rows_lists_check(fn, cout, channels, nullptr, nrows, err);
  if (rc != SMPQ_OK) return rc;
  const int8_t* sv = static_cast<const int8_t*>(save);
  for (int i = 0; i < nrows; ++i)
    for (int l = 0; l < limbs; ++l)
      for (long long m = 0; m < pixels; ++m)
        yq[((long long)l * pixels + m) * cout + channels[i]] = sv[((long long)i * limbs + l) * pixels + m];
  return SMPQ_OK;
}

}  // namespace smpq
