// Stand-alone host check of the exact8 rows patch's native twins (csrc/trial_row_host.h, which
// smpq_trial_rows_patch_x8_host / smpq_trial_rows_restore_x8_host wrap) under AddressSanitizer and
// UndefinedBehaviorSanitizer. No GPU, no Python:
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/trial_rows_x8_sanitize.cpp -o build/trial_rows_x8_sanitize && build/trial_rows_x8_sanitize
//
// Every operand, the two lists, the n-slot save area and the n status words are exact-size heap
// blocks, so a byte read or written outside them is reported. Shapes: [64, 64, 1, 1], [64, 64, 3, 3]
// and the longest row the kernel takes ([16, 512, 3, 3], K = 4608); both semantics; with and without
// an offset array; an unsorted list with the first and the last channel and mixed bits (8, 6, 4, 2);
// n = 1 and n = cout; a constant row, an off-grid row and a row that needs an offset in the list.
// What the arithmetic must give is tests/test_search_host.py's business; here the status words, the
// untouched rows and the restore are checked. Then every argument check.
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
  std::vector<int32_t> offset;
  std::vector<float> wscale, col_scale;
  bool operator==(const Operand& o) const {
    return codes == o.codes && offset == o.offset && wscale == o.wscale && col_scale == o.col_scale;
  }
};

// rows 7 (constant), 2 (off the grid) and 4 (codes 150..165 at 4 bits: needs an offset)
static int expected(int c, int b, bool with_offset) {
  if (c == 7) return 1;
  if (c == 2) return 3;
  if (c == 4 && b == 4 && !with_offset) return 4;
  return -1;  // 0, or 4 when the row happens to need an offset and there is none
}

static void run_list(const std::vector<float>& w, int cout, int cin, int kh, int kw, int sem,
                     const std::vector<int32_t>& chans, const std::vector<int32_t>& bits, const Operand& start,
                     const std::vector<float>& a, bool with_offset) {
  const int K = cin * kh * kw, n = (int)chans.size();
  const size_t slot = SMPQ_TRIAL_SAVE_HEADER + (size_t)K;
  std::string err;
  Operand got = start;
  int32_t* ch = new int32_t[n];
  int32_t* bt = new int32_t[n];
  int32_t* status = new int32_t[n]();
  int8_t* save = new int8_t[(size_t)n * slot]();
  std::copy(chans.begin(), chans.end(), ch);
  std::copy(bits.begin(), bits.end(), bt);
  int32_t* off = with_offset ? got.offset.data() : nullptr;
  int rc = smpq::trial_rows_patch_x8_host(w.data(), cout, cin, kh, kw, ch, bt, n, sem, a.data(), got.codes.data(), off,
                                          got.wscale.data(), got.col_scale.data(), save, status, &err);
  CHECK(rc == SMPQ_OK);
  std::vector<bool> listed(cout, false);
  for (int i = 0; i < n; ++i) {
    const int c = ch[i], want = expected(c, bt[i], with_offset);
    listed[c] = true;
    CHECK(want < 0 ? (status[i] == 0 || (status[i] == 4 && !with_offset)) : status[i] == want);
    const int8_t* s = save + (size_t)i * slot;
    int32_t o = 0;
    std::memcpy(&o, s + 8, 4);
    CHECK(o == (with_offset ? start.offset[c] : 0));
    CHECK(std::memcmp(s + SMPQ_TRIAL_SAVE_HEADER, start.codes.data() + (size_t)c * K, K) == 0);
    if (status[i] != 0) {  // the row stays as it is
      CHECK(std::memcmp(got.codes.data() + (size_t)c * K, start.codes.data() + (size_t)c * K, K) == 0);
      CHECK(got.wscale[c] == start.wscale[c] && got.col_scale[c] == start.col_scale[c] && got.offset[c] == start.offset[c]);
    } else {
      CHECK(got.col_scale[c] == got.wscale[c] * a[c]);
    }
  }
  for (int c = 0; c < cout; ++c)
    if (!listed[c]) CHECK(std::memcmp(got.codes.data() + (size_t)c * K, start.codes.data() + (size_t)c * K, K) == 0);
  rc = smpq::trial_rows_restore_x8_host(cout, K, ch, n, got.codes.data(), off, got.wscale.data(), got.col_scale.data(),
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
  for (int i = 0; i < K; ++i) w[(size_t)7 * K + i] = 0.25f;                                   // a constant row
  for (int i = 0; i < K; ++i) w[(size_t)2 * K + i] = 1000.f + 1e-3f * (float)(i % 64);       // an off-grid row
  for (int i = 0; i < K; ++i) w[(size_t)4 * K + i] = 1.0f + 0.1f * (float)(i % 64) / 63.0f;  // needs an offset
  std::vector<float> a(cout);
  for (int c = 0; c < cout; ++c) a[c] = 0.5f + 0.01f * (float)c;
  const int32_t pick[] = {4, 6, 8, 2};
  Operand start;
  start.codes.resize((size_t)cout * K);
  for (int8_t& v : start.codes) v = (int8_t)bd(rng);
  start.offset.assign(cout, -3);
  start.wscale.assign(cout, 0.5f);
  start.col_scale.assign(cout, 0.75f);
  for (int sem = 0; sem <= 1; ++sem)
    for (int with_offset = 0; with_offset <= 1; ++with_offset) {
      std::vector<int32_t> chans = {cout - 1, 3, 7, 0, 4, 2, cout / 2};
      std::vector<int32_t> bits = {4, 6, 8, 2, 4, 8, 6};
      run_list(w, cout, cin, kh, kw, sem, chans, bits, start, a, with_offset != 0);
      run_list(w, cout, cin, kh, kw, sem, {cout - 1}, {4}, start, a, with_offset != 0);  // n = 1
      std::vector<int32_t> all(cout);                                                      // n = cout
      std::iota(all.begin(), all.end(), 0);
      std::shuffle(all.begin(), all.end(), rng);
      std::vector<int32_t> allbits;
      for (int i = 0; i < cout; ++i) allbits.push_back(all[i] == 4 ? 4 : pick[i % 4]);
      run_list(w, cout, cin, kh, kw, sem, all, allbits, start, a, with_offset != 0);
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
  int32_t st[3] = {0, 0, 0}, off[3] = {0, 0, 0};
  int32_t ch[3] = {5, 63, 0}, bits[3] = {8, 4, 2};
  int32_t dup[3] = {5, 63, 5}, high[3] = {5, 64, 0}, neg[3] = {5, -1, 0}, bit0[3] = {8, 0, 2}, bit9[3] = {8, 4, 9};
  using smpq::trial_rows_patch_x8_host;
  using smpq::trial_rows_restore_x8_host;
  CHECK(trial_rows_patch_x8_host(nullptr, 64, 64, 1, 1, ch, bits, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, nullptr, bits, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, nullptr, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bits, 3, 0, f, nullptr, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bits, 3, 0, f, b, off, f, f, nullptr, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bits, 3, 0, f, b, off, f, f, b, nullptr, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bits, 0, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bits, 65, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bits, 3, 2, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bits, 3, 0, f, b, off, f, f, b + 1, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 32, 1, 1, ch, bits, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_SHAPE);
  CHECK(trial_rows_patch_x8_host(f, 64, 576, 3, 3, ch, bits, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_SHAPE);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, dup, bits, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, high, bits, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, neg, bits, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bit0, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_BITS);
  CHECK(trial_rows_patch_x8_host(f, 64, 64, 1, 1, ch, bit9, 3, 0, f, b, off, f, f, b, st, &err) == SMPQ_E_BITS);
  CHECK(err.find("smpq_trial_rows_patch_x8") == 0);
  CHECK(trial_rows_restore_x8_host(64, 64, nullptr, 3, b, off, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_x8_host(64, 64, ch, 3, nullptr, off, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_x8_host(64, 64, ch, 0, b, off, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_x8_host(64, 64, ch, 65, b, off, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_x8_host(64, 64, dup, 3, b, off, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_x8_host(64, 64, high, 3, b, off, f, f, b, &err) == SMPQ_E_INVALID);
  CHECK(trial_rows_restore_x8_host(64, 32, ch, 3, b, off, f, f, b, &err) == SMPQ_E_SHAPE);
  CHECK(trial_rows_restore_x8_host(64, 4672, ch, 3, b, off, f, f, b, &err) == SMPQ_E_SHAPE);
  CHECK(err.find("smpq_trial_rows_restore_x8") == 0);
  CHECK(st[0] == 0 && st[1] == 0 && st[2] == 0 && b[0] == 0 && f[0] == 0.f && f[3] == 3.f && off[1] == 0);
  std::printf(failures ? "trial_rows_x8_sanitize: %d check(s) failed\n" : "trial_rows_x8_sanitize: ok\n", failures);
  return failures ? 1 : 0;
}
