// Host twins of the trial row patch (include/smpq.h, "trial row patch"): native C++, no HIP, so a
// stand-alone host program (tools/trial_row_sanitize.cpp) can compile them under a sanitizer.
// quant.hip wraps them as smpq_trial_row_patch_host / smpq_trial_row_restore_host. The arithmetic
// restates quantize_row_host and pack_weights_ex_kernel (lw >= 2) of quant.hip; FP contraction off.
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
                           const void* col_scale, const void* save, const void* status, std::string* err) {
  if (!w || !bn_a || !codes || !wscale || !col_scale || !save || !status) {
    *err = "smpq_trial_row_patch: null pointer";
    return SMPQ_E_INVALID;
  }
  if (cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) {
    *err = "smpq_trial_row_patch: sizes must be positive";
    return SMPQ_E_INVALID;
  }
  if (wlimbs < 2 || wlimbs > 3) {
    *err = "smpq_trial_row_patch: wlimbs must be 2 or 3";
    return SMPQ_E_INVALID;
  }
  if (channel < 0 || channel >= cout) {
    *err = "smpq_trial_row_patch: channel outside [0, cout)";
    return SMPQ_E_INVALID;
  }
  if (semantics != SMPQ_QSEM_CPU && semantics != SMPQ_QSEM_DEVICE) {
    *err = "smpq_trial_row_patch: semantics must be SMPQ_QSEM_CPU or SMPQ_QSEM_DEVICE";
    return SMPQ_E_INVALID;
  }
  if ((uintptr_t)save & 3) {
    *err = "smpq_trial_row_patch: save area must be 4-byte aligned";
    return SMPQ_E_INVALID;
  }
  if (cin % 64 != 0 || (long long)cin * kh * kw > SMPQ_TRIAL_MAX_K) {
    *err = "smpq_trial_row_patch: cin must be a multiple of 64 and K at most SMPQ_TRIAL_MAX_K";
    return SMPQ_E_SHAPE;
  }
  if (bits < 1 || bits > 16) {
    *err = "smpq_trial_row_patch: bits outside 1..16";
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

inline int trial_row_patch_host(const float* w, int cout, int cin, int kh, int kw, int channel, int bits,
                                int semantics, int wlimbs, const float* bn_a, int8_t* codes, float* wscale,
                                float* col_scale, void* save, int32_t* status, std::string* err) {
  const int rc = trial_row_check(w, cout, cin, kh, kw, channel, bits, semantics, wlimbs, bn_a, codes, wscale,
                                 col_scale, save, status, err);
  if (rc != SMPQ_OK) return rc;
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
    return SMPQ_OK;
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

}  // namespace smpq
