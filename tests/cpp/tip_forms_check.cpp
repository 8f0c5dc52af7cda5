// The tip forms of engine creation (libsbn_amd/csrc/mi_phylo_tip_forms.h), checked without a
// device against their definition written out as tables: compact state -> byte / mask / code /
// partial row for the states 0..3, the gap and values outside the range; partial row -> mask ->
// code for one-hot rows, all ones, other 0/1 patterns (a mask but no code) and real-valued rows
// (no mask); the 20-state row -> compact state check.  Rows are heap blocks of exactly their
// size, so built with -fsanitize=address,undefined a read past a row stops the program.
//   g++ -std=c++17 -g -fsanitize=address,undefined tests/cpp/tip_forms_check.cpp -o check && ./check
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../libsbn_amd/csrc/mi_phylo_tip_forms.h"

using namespace miphylo;

namespace {

int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      failures++;                        \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
    }                                    \
  } while (0)

void states_to_forms() {
  const uint8_t masks[5] = {1, 2, 4, 8, 15}, codes[5] = {0, 16, 32, 48, 64};
  const double rows[5][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}, {1, 1, 1, 1}};
  const int32_t lo = std::numeric_limits<int32_t>::min(), hi = std::numeric_limits<int32_t>::max();
  for (int states : {4, 20}) {
    for (int32_t v = 0; v < states; v++) CHECK(tip_state(v, states) == v, "states %d value %d", states, v);
    for (int32_t v : {lo, -1000, -1, states, states + 1, 127, 128, 255, 256, hi})
      CHECK(tip_state(v, states) == states, "states %d value %d", states, v);
  }
  for (int32_t v : {0, 1, 2, 3, 4, 5, -1, 64, 255, lo, hi}) {
    const int c = tip_state(v, 4), want = (v >= 0 && v < 4) ? v : 4;
    CHECK(c == want, "value %d", v);
    CHECK(tip_mask(c) == masks[want], "value %d", v);
    CHECK(tip_code(c) == codes[want], "value %d", v);
    for (int k = 0; k < 4; k++) CHECK(tip_partial(c, k) == rows[want][k], "value %d entry %d", v, k);
  }
}

void partials_to_forms() {
  // every 0/1 row: its mask is its bits, and it has a code exactly when it is one-hot or all ones
  for (int bits = 0; bits < 16; bits++) {
    std::vector<double> row(4);
    for (int x = 0; x < 4; x++) row[x] = (bits >> x) & 1 ? 1.0 : 0.0;
    const uint8_t m = tip_mask_of_partials(row.data());
    CHECK(m == bits, "row %d", bits);
    uint8_t want = kTipNoForm;
    if (bits == 1) want = 0;
    if (bits == 2) want = 16;
    if (bits == 4) want = 32;
    if (bits == 8) want = 48;
    if (bits == 15) want = 64;
    CHECK(tip_code_of_mask(m) == want, "row %d", bits);
    // ... and the row a compact state expands to comes back as that state's mask and code
    for (int c = 0; c <= 4; c++)
      if (tip_mask(c) == bits)
        for (int k = 0; k < 4; k++) CHECK(tip_partial(c, k) == row[k], "state %d entry %d", c, k);
  }
  // -0.0 is 0; anything else beside 0 and 1 leaves the row without a mask, wherever it stands
  std::vector<double> zero{1.0, -0.0, 0.0, 0.0};
  CHECK(tip_mask_of_partials(zero.data()) == 1, "-0.0");
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (double v : {0.25, 0.5, 0.999999, 1.0000001, 2.0, -1.0, 1e-300, nan, inf})
    for (int at = 0; at < 4; at++)
      for (double rest : {0.0, 1.0}) {
        std::vector<double> row(4, rest);
        row[at] = v;
        CHECK(tip_mask_of_partials(row.data()) == kTipNoForm, "value %g at %d", v, at);
      }
  CHECK(tip_code_of_mask(kTipNoForm) == kTipNoForm, "no mask, no code");
}

void rows_to_states() {
  for (int states : {4, 20}) {
    for (int c = 0; c < states; c++) {
      std::vector<double> row(states, 0.0);
      row[c] = 1.0;
      CHECK(tip_state_of_partials(row.data(), states) == c, "states %d one-hot %d", states, c);
      row[c] = 0.5;
      CHECK(tip_state_of_partials(row.data(), states) == -1, "states %d real value at %d", states, c);
      row[c] = 1.0;
      row[(c + 1) % states] = 1.0;
      CHECK(tip_state_of_partials(row.data(), states) == -1, "states %d two ones at %d", states, c);
    }
    std::vector<double> row(states, 1.0);
    CHECK(tip_state_of_partials(row.data(), states) == states, "states %d all ones", states);
    row[states - 1] = 0.0;
    CHECK(tip_state_of_partials(row.data(), states) == -1, "states %d all ones but the last", states);
    row[states - 1] = 2.0;
    CHECK(tip_state_of_partials(row.data(), states) == -1, "states %d a 2 among ones", states);
    std::vector<double> none(states, 0.0);
    CHECK(tip_state_of_partials(none.data(), states) == -1, "states %d all zeros", states);
  }
}

}  // namespace

int main() {
  states_to_forms();
  partials_to_forms();
  rows_to_states();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
