// Stand-alone host check of the trial rows patch's native twins (csrc/trial_row_host.h, which
// smpq_trial_rows_patch_host / smpq_trial_rows_restore_host wrap) under AddressSanitizer and
// UndefinedBehaviorSanitizer. No GPU, no Python:
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/trial_rows_sanitize.cpp -o build/trial_rows_sanitize && build/trial_rows_sanitize
//
// Every operand, the two lists, the n-slot save area and the n status words are exact-size heap
// blocks, so a byte read or written outside them is reported. Shapes: [64, 64, 1, 1], [64, 64, 3, 3]
// and the longest row the kernel takes ([16, 512, 3, 3], K = 4608); LW 2 and 3; both semantics; an
// unsorted list with the first and the last channel and mixed bits (8, 6, 4, 2); n = 1 and n = cout;
// a constant row in the middle of a list; an off-grid row. Each result is compared with the
// single-row twin called once per row on a copy, slot by slot. Then every argument check.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
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

struct Operand {
  std::vector<int8_t> codes;
  std::vector<float> wscale, col_scale;
  bool operator==(const Operand& o) const {
    return codes == o.codes && wscale == o.wscale && col_scale == o.col_scale;
  }
};

static void run_list(const std::vector<float>& w, int cout, int cin, int kh, int kw, int lw, int sem,
                     const std::vector<int32_t>& chans, const std::vector<int32_t>& bits, const Operand& start,
                     const std::vector<float>& a, const std::vector<bool>& constant) {
  const int K = cin * kh * kw, n = (int)chans.size();
  const size_t slot = SMPQ_TRIAL_SAVE_HEADER + (size_t)lw * K;
  std::string err;
  // the single-row twin, once per row, on a copy
  Operand want = start;
  std::vector<std::vector<int8_t>> slots;
  for (int i = 0; i < n; ++i) {
    std::vector<int8_t> sv(slot, 0);
    int32_t st = 0;
    CHECK(smpq::trial_row_patch_host(w.data(), cout, cin, kh, kw, chans[i], bits[i], sem, lw, a.data(),
                                     want.codes.data(), want.wscale.data(), want.col_scale.data(), sv.data(), &st,
                                     &err) == SMPQ_OK);
    CHECK((st == 1) == constant[chans[i]]);
    slots.push_back(sv);
  }
  Operand got = start;
  // exact-size heap blocks for what the call indexes by i
  int32_t* ch = new int32_t[n];
  int32_t* bt = new int32_t[n];
  int32_t* status = new int32_t[n]();
  int8_t* save = new int8_t[(size_t)n * slot]();
  std::copy(chans.begin(), chans.end(), ch);
  std::copy(bits.begin(), bits.end(), bt);
  int rc = smpq::trial_rows_patch_host(w.data(), cout, cin, kh, kw, ch, bt, n, sem, lw, a.data(), got.codes.data(),
                                       got.wscale.data(), got.col_scale.data(), save, status, &err);
  CHECK(rc == SMPQ_OK);
  CHECK(got == want);
  for (int i = 0; i < n; ++i) {
    CHECK(status[i] == (constant[chans[i]] ? 1 : 0));
    const int8_t* s = save + (size_t)i * slot;
    CHECK(std::memcmp(s, slots[i].data(), 8) == 0);
    CHECK(std::memcmp(s + SMPQ_TRIAL_SAVE_HEADER, slots[i].data() + SMPQ_TRIAL_SAVE_HEADER, (size_t)lw * K) == 0);
  }
  rc = smpq::trial_rows_restore_host(cout, K, ch, n, lw, got.codes.data(), got.wscale.data(), got.col_scale.data(),
                                     save, &err);
  CHECK(rc == SMPQ_OK);
  CHECK(got == start);
  delete[] ch;
  delete[] bt;
  delete[] status;
  delete[] save;
}

static void run_shape(int cout, int cin, int kh, int kw, std::mt19937& rng) {
  const int K = cin * kh * kw;
  std::normal_distribution<float> nd(0.f, 0.05f);
  std::uniform_int_distribution<int> bd(-128, 127);
  std::vector<float> w((size_t)cout * K);
  for (float& v : w) v = nd(rng);
  std::vector<bool> constant(cout, false);
  constant[7] = true;
  for (int i = 0; i < K; ++i) w[(size_t)7 * K + i] = 0.25f;                      // a constant row
  for (int i = 0; i < K; ++i) w[(size_t)2 * K + i] = 1000.f + 1e-3f * (float)i;  // an off-grid row
  std::vector<float> a(cout);
  for (int c = 0; c < cout; ++c) a[c] = 0.5f + 0.01f * (float)c;
  const int32_t pick[] = {8, 6, 4, 2};
  for (int lw = 2; lw <= 3; ++lw) {
    Operand start;
    start.codes.resize((size_t)lw * cout * K);
    for (int8_t& v : start.codes) v = (int8_t)bd(rng);
    start.wscale.assign(cout, 0.5f);
    start.col_scale.assign(cout, 0.75f);
    for (int sem = 0; sem <= 1; ++sem) {
      // unsorted, first and last channel, the constant row in the middle, the off-grid row
      std::vector<int32_t> chans = {cout - 1, 3, 7, 0, 2, cout / 2};
      std::vector<int32_t> bits;
      for (size_t i = 0; i < chans.size(); ++i) bits.push_back(pick[i % 4]);
      run_list(w, cout, cin, kh, kw, lw, sem, chans, bits, start, a, constant);
      run_list(w, cout, cin, kh, kw, lw, sem, {cout - 1}, {4}, start, a, constant);  // n = 1
      std::vector<int32_t> all(cout);                                                  // n = cout
      std::iota(all.begin(), all.end(), 0);
      std::shuffle(all.begin(), all.end(), rng);
      std::vector<int32_t> allbits;
      for (int i = 0; i < cout; ++i) allbits.push_back(pick[i % 4]);
      run_list(w, cout, cin, kh, kw, lw, sem, all, allbits, start, a, constant);
    }
  }
}

int main() {
  std::mt19937 rng(7);
  run_shape(64, 64, 1, 1, rng);
  run_shape(64, 64, 3, 3, rng);
  run_shape(16, 512, 3, 3, rng);
  // argument checks: nothing behind the pointers is read or written (they are far too small)
  std::string err;
  float f[4] = {0, 1, 2, 3};
  alignas(16) int8_t b[8] = {0};
  int32_t st[3] = {0, 0, 0};
  int32_t ch[3] = {5, 63, 0}, bits[3] = {8, 4, 2};
  int32_t dup[3] = {5, 63, 5}, high[3] = {5, 64, 0}, neg[3] = {5, -1, 0}, bit0[3] = {8, 0, 2}, bit17[3] = {8, 4, 17};
  using smpq::trial_rows_patch_host;
  using smpq::trial_rows_restore_host;
  CHECK(trial_rows_patch_host(nullptr, 64, 64, 1, 1, ch, bits, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, nullptr, bits, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, nullptr, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 3, 0, 2, f, b, f, f, nullptr, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 3, 0, 2, f, b, f, f, b, nullptr, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 0, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 65, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(err.find("smpq_trial_rows_patch") == 0);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 3, 0, 1, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 3, 0, 4, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 3, 2, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bits, 3, 0, 2, f, b, f, f, b + 1, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 32, 1, 1, ch, bits, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_SHAPE);
  CHECK(trial_rows_patch_host(f, 64, 576, 3, 3, ch, bits, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_SHAPE);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, dup, bits, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, high, bits, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, neg, bits, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bit0, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_BITS);
  CHECK(trial_rows_patch_host(f, 64, 64, 1, 1, ch, bit17, 3, 0, 2, f, b, f, f, b, st, &err) == SMPQ_E_BITS);
  CHECK(err.find("smpq_trial_rows_patch") == 0);
  CHECK(trial_rows_restore_host(64, 64, nullptr, 3, 2, b, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_host(64, 64, ch, 3, 2, nullptr, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_host(64, 64, ch, 0, 2, b, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_host(64, 64, ch, 65, 2, b, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_host(64, 64, ch, 3, 1, b, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_host(64, 64, dup, 3, 2, b, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_host(64, 64, high, 3, 2, b, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_host(64, 32, ch, 3, 2, b, f, f, b, &err) == SMPQ_E_SHAPE);
  CHECK(trial_rows_restore_host(64, 4672, ch, 3, 2, b, f, f, b, &err) == SMPQ_E_SHAPE);
  CHECK(err.find("smpq_trial_rows_restore") == 0);
  CHECK(st[0] == 0 && st[1] == 0 && st[2] == 0 && b[0] == 0 && f[0] == 0.f && f[3] == 3.f);
  std::printf(failures ? "trial_rows_sanitize: %d check(s) failed\n" : "trial_rows_sanitize: ok\n", failures);
  return failures ? 1 : 0;
}
