// Stand-alone host check of the trial row patch's native twins (csrc/trial_row_host.h, which
// smpq_trial_row_patch_host / smpq_trial_row_restore_host wrap) under AddressSanitizer and
// UndefinedBehaviorSanitizer. No GPU, no Python:
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/trial_row_sanitize.cpp -o build/trial_row_sanitize && build/trial_row_sanitize
//
// Every operand, the save area and the status word are exact-size heap blocks, so a byte read or
// written outside them is reported. Shapes: [64, 64, 1, 1], [64, 64, 3, 3], [128, 256, 1, 1] and the
// longest row the kernel takes ([16, 512, 3, 3], K = 4608); LW 2 and 3; 16, 8, 6, 4, 2 and 1 bits;
// both semantics; first and last channel; a constant row; an off-grid row; every argument check.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../semilayer-wise-mixed-precision-quantization_amd/csrc/trial_row_host.h"

static int failures = 0;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void run_shape(int cout, int cin, int kh, int kw, std::mt19937& rng) {
  const int K = cin * kh * kw;
  std::normal_distribution<float> nd(0.f, 0.05f);
  std::uniform_int_distribution<int> bd(-128, 127);
  std::vector<float> w((size_t)cout * K);
  for (float& v : w) v = nd(rng);
  for (int i = 0; i < K; ++i) w[(size_t)1 * K + i] = 0.25f;                      // a constant row
  for (int i = 0; i < K; ++i) w[(size_t)2 * K + i] = 1000.f + 1e-3f * (float)i;  // an off-grid row
  std::vector<float> a(cout, 1.5f);
  std::string err;
  for (int lw = 2; lw <= 3; ++lw) {
    std::vector<int8_t> codes((size_t)lw * cout * K);
    for (int8_t& v : codes) v = (int8_t)bd(rng);
    std::vector<float> wscale(cout, 0.5f), col_scale(cout, 0.75f);
    const std::vector<int8_t> codes0 = codes;
    std::vector<int8_t> save(SMPQ_TRIAL_SAVE_HEADER + (size_t)lw * K);
    const int chans[] = {0, 1, 2, cout - 1};
    const int bits[] = {16, 8, 6, 4, 2, 1};
    for (int c : chans)
      for (int b : bits)
        for (int sem = 0; sem <= 1; ++sem) {
          int32_t* status = new int32_t[1]{0};
          int rc = smpq::trial_row_patch_host(w.data(), cout, cin, kh, kw, c, b, sem, lw, a.data(), codes.data(),
                                              wscale.data(), col_scale.data(), save.data(), status, &err);
          CHECK(rc == SMPQ_OK);
          CHECK((*status == 1) == (c == 1));
          if (c == 1) CHECK(codes == codes0);
          else CHECK(col_scale[c] == wscale[c] * a[c]);
          rc = smpq::trial_row_restore_host(cout, K, c, lw, codes.data(), wscale.data(), col_scale.data(), save.data(),
                                            &err);
          CHECK(rc == SMPQ_OK);
          CHECK(codes == codes0 && wscale[c] == 0.5f && col_scale[c] == 0.75f);
          delete[] status;
        }
  }
}

int main() {
  std::mt19937 rng(7);
  run_shape(64, 64, 1, 1, rng);
  run_shape(64, 64, 3, 3, rng);
  run_shape(128, 256, 1, 1, rng);
  run_shape(16, 512, 3, 3, rng);
  // argument checks: nothing is read or written
  std::string err;
  float f[4] = {0, 1, 2, 3};
  int8_t b[4] = {0};
  int32_t st = 0;
  using smpq::trial_row_patch_host;
  CHECK(trial_row_patch_host(nullptr, 64, 64, 1, 1, 0, 4, 0, 2, f, b, f, f, f, &st, &err) == SMPQ_E_INVALID);
  CHECK(trial_row_patch_host(f, 64, 64, 1, 1, 0, 4, 0, 1, f, b, f, f, f, &st, &err) == SMPQ_E_INVALID);
  CHECK(trial_row_patch_host(f, 64, 64, 1, 1, 0, 4, 0, 4, f, b, f, f, f, &st, &err) == SMPQ_E_INVALID);
  CHECK(trial_row_patch_host(f, 64, 64, 1, 1, 64, 4, 0, 2, f, b, f, f, f, &st, &err) == SMPQ_E_INVALID);
  CHECK(trial_row_patch_host(f, 64, 64, 1, 1, 0, 4, 2, 2, f, b, f, f, f, &st, &err) == SMPQ_E_INVALID);
  CHECK(trial_row_patch_host(f, 64, 32, 1, 1, 0, 4, 0, 2, f, b, f, f, f, &st, &err) == SMPQ_E_SHAPE);
  CHECK(trial_row_patch_host(f, 64, 576, 3, 3, 0, 4, 0, 2, f, b, f, f, f, &st, &err) == SMPQ_E_SHAPE);
  CHECK(trial_row_patch_host(f, 64, 64, 1, 1, 0, 0, 0, 2, f, b, f, f, f, &st, &err) == SMPQ_E_BITS);
  CHECK(trial_row_patch_host(f, 64, 64, 1, 1, 0, 17, 0, 2, f, b, f, f, f, &st, &err) == SMPQ_E_BITS);
  CHECK(smpq::trial_row_restore_host(64, 64, 0, 2, nullptr, f, f, f, &err) == SMPQ_E_INVALID);
  CHECK(smpq::trial_row_restore_host(64, 32, 0, 2, b, f, f, f, &err) == SMPQ_E_SHAPE);
  CHECK(st == 0);
  std::printf(failures ? "trial_row_sanitize: %d check(s) failed\n" : "trial_row_sanitize: ok\n", failures);
  return failures ? 1 : 0;
}
