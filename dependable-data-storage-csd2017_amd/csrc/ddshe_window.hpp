// Sliding-window schedule of the modexp ladder (k_modexp_pre / k_modexp_ladder, driven by modexp_device in
// ddshe_paillier.cpp). Host arithmetic only, no HIP: host_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <vector>

#include "bn_host.hpp"

namespace ddshe {
namespace host {

// Sliding-window schedule of a uniform exponent E (left to right): sched[0] = index of the
// leading window's odd power, then (nsq << 16) | (idx + 1) per later window (idx + 1 == 0:
// trailing squarings only). Returns the number of odd powers the table must hold.
// bench.py's window_counts mirrors this function (its squaring and multiply counts are checked
// against it by tests/test_host_helpers.py): change the two together.
inline int window_schedule(const bn::Limbs& E, std::vector<uint32_t>* sched) {
  sched->clear();
  const int nb = (int)bn::bit_length(E);
  if (nb == 0) return 1;
  auto bit = [&](int i) { return (E[(size_t)i >> 5] >> (i & 31)) & 1u; };
  // window width minimising table + multiplies (table of 2^(w-1) odd powers per row)
  const int w = nb <= 24 ? 1 : nb <= 80 ? 3 : nb <= 240 ? 4 : 5;
  int i = nb - 1;
  uint32_t pending_sq = 0;
  bool first = true;
  while (i >= 0) {
    if (!bit(i)) {
      ++pending_sq;
      --i;
      continue;
    }
    int j = std::max(i - w + 1, 0);
    while (!bit(j)) ++j;  // window [i..j] ends on a set bit
    uint32_t v = 0;
    for (int k = i; k >= j; --k) v = (v << 1) | bit(k);
    const uint32_t idx = (v - 1) / 2;
    if (first) {
      sched->push_back(idx);
      first = false;
    } else {
      pending_sq += (uint32_t)(i - j + 1);
      sched->push_back((pending_sq << 16) | (idx + 1));
    }
    pending_sq = 0;
    i = j - 1;
  }
  while (pending_sq > 0) {  // trailing zero bits: squarings only, <= 0xFFFF per entry
    const uint32_t c = std::min<uint32_t>(pending_sq, 0xFFFF);
    sched->push_back(c << 16);
    pending_sq -= c;
  }
  return 1 << (w - 1);
}

}  // namespace host
}  // namespace ddshe
