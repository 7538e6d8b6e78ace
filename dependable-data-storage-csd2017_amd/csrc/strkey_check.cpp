// CPU check of the grouping by strings (dds_col_fold_by_str: label_by_str and fold_by_str_device of
// ddshe_keyed.cpp driving the kernels of ddshe_strkey.hip). No device code: a model of the passes built on the
// shared primitives of ddshe_strkey.hpp -- the salted digest truncated to the pass's bits, a stable sort of the
// participating rows by it, the segment heads, the adjacent verification, the salt loop, the groups ordered by their
// first rows -- against a std::map<std::string, ...> grouping of the same rows, over seeded tables with empty
// strings, proper prefixes, equal-length strings that differ in the last byte only, 300-byte strings and bytes
// >= 0x80, with dead rows, short rows and a mask. Then the first pass truncated to 1, 4 and 8 bits: its segments
// interleave distinct strings (A, B, A, B), the verification must reject it, and the second pass must give the
// exact grouping; and a variant that truncates every pass, which must end in the give-up result rather than in a
// grouping. Salt 0 must equal the table's own str_digest (ddshe_launch.hpp), other salts must not.
// Exits non-zero on the first failed check, naming it; prints "ok <case>" lines and "strkey_check: all passed"
// (tests/test_strkey_check.py).
#include <algorithm>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "check_util.hpp"
#include "ddshe_launch.hpp"  // str_digest only
#include "ddshe_strkey.hpp"

using namespace ddshe;
using namespace ddshe::check;

namespace {

Lcg g_rng{0x243F6A8885A308D3ull};

struct Row {
  bool col_live = true, tab_live = true, in_mask = true;
  std::vector<std::string> elems;
};

struct Grouping {
  bool ok = false;  // false: the salt loop gave up
  int passes = 0;
  std::vector<uint32_t> first;               // per group, in the groups' order
  std::vector<std::vector<uint32_t>> rows;  // the group's rows, ascending
};

const uint8_t* bytes(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

// the passes of label_by_str and the order of fold_by_str_device; all_bits: every pass sorts by that many bits
// (the give-up variant), else only the first (DDSHE_STRKEY_BITS)
Grouping model(const std::vector<Row>& tab, uint64_t position, int first_bits, bool truncate_all) {
  const size_t n = tab.size();
  Grouping out;
  for (int pass = 0; pass < kStrKeyPasses; ++pass) {
    out.passes = pass + 1;
    const int bits = truncate_all ? first_bits : strkey_pass_bits(pass, first_bits);
    std::vector<uint8_t> valid(n);
    std::vector<int64_t> key(n);
    for (size_t r = 0; r < n; ++r) {
      const Row& w = tab[r];
      valid[r] = strkey_takes_part(w.col_live, w.tab_live, (uint32_t)w.elems.size(), position, w.in_mask);
      key[r] = 0;
      if (valid[r]) {
        const std::string& s = w.elems[position];
        key[r] = strkey_sort_key(strkey_digest(bytes(s), s.size(), (uint64_t)pass), bits);
      }
    }
    // launch_ope_order: invalid rows first, then ascending keys, equal keys in row order
    std::vector<uint32_t> perm(n);
    for (size_t r = 0; r < n; ++r) perm[r] = (uint32_t)r;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
      if (valid[a] != valid[b]) return valid[a] < valid[b];
      return valid[a] && key[a] < key[b];
    });
    // launch_ope_rank's heads and k_strkey_verify's adjacent comparisons
    std::vector<size_t> starts;
    size_t mismatches = 0;
    for (size_t j = 0; j < n; ++j) {
      const uint32_t r = perm[j];
      if (!valid[r]) continue;
      const bool pv = j > 0 && valid[perm[j - 1]];
      if (strkey_is_head(true, pv, key[r], pv ? key[perm[j - 1]] : 0)) {
        starts.push_back(j);
        continue;
      }
      if (tab[r].elems[position] != tab[perm[j - 1]].elems[position]) ++mismatches;
    }
    if (mismatches) continue;  // a collision: the next salt
    // verified: first rows, the groups ordered by them
    const size_t ng = starts.size();
    std::vector<uint32_t> ord(ng);
    for (size_t g = 0; g < ng; ++g) ord[g] = (uint32_t)g;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return perm[starts[a]] < perm[starts[b]]; });
    for (size_t g = 0; g < ng; ++g) {
      const size_t s = ord[g], a = starts[s], e = s + 1 < ng ? starts[s + 1] : n;
      out.first.push_back(perm[a]);
      out.rows.emplace_back(perm.begin() + a, perm.begin() + e);
    }
    out.ok = true;
    return out;
  }
  return out;
}

// the reference: a map by text, groups in order of first occurrence
Grouping reference(const std::vector<Row>& tab, uint64_t position) {
  std::map<std::string, size_t> code;
  Grouping out;
  out.ok = true;
  for (size_t r = 0; r < tab.size(); ++r) {
    const Row& w = tab[r];
    if (!w.col_live || !w.tab_live || !w.in_mask || w.elems.size() <= position) continue;
    auto it = code.find(w.elems[position]);
    if (it == code.end()) {
      it = code.emplace(w.elems[position], out.first.size()).first;
      out.first.push_back((uint32_t)r);
      out.rows.emplace_back();
    }
    out.rows[it->second].push_back((uint32_t)r);
  }
  return out;
}

void same(const Grouping& got, const Grouping& want, const std::string& tag) {
  need(got.ok, tag + ": the model gave up");
  need(got.first == want.first, tag + ": first rows");
  need(got.rows == want.rows, tag + ": group rows");
}

std::string rnd_string(size_t len, bool high) {
  std::string s(len, '\0');
  for (auto& c : s) c = (char)(high ? 0x80 | (g_rng.rnd32() & 0x7F) : 'a' + g_rng.rnd32() % 26);
  return s;
}

// the pool of texts the seeded tables draw from: "", proper prefixes, equal lengths differing in the last byte,
// 300-byte strings, bytes >= 0x80, "7" next to "07"
std::vector<std::string> pool() {
  std::vector<std::string> p = {"", "a", "ab", "abc", "abd", "7", "07", "None", "true"};
  const std::string long0 = rnd_string(300, false);
  std::string long1 = long0;
  long1[299] = (char)(long1[299] == 'z' ? 'y' : long1[299] + 1);
  p.push_back(long0);
  p.push_back(long1);
  p.push_back(long0.substr(0, 299));
  p.push_back("caf\xc3\xa9");
  p.push_back("caf\xc3\xa8");
  p.push_back(std::string("\x80\xff\x00\x81", 4));
  p.push_back(std::string("\x80\xff\x00\x82", 4));
  for (int i = 0; i < 24; ++i) p.push_back(rnd_string(1 + g_rng.rnd32() % 12, i % 3 == 0));
  return p;
}

std::vector<Row> table(const std::vector<std::string>& p, size_t n, uint64_t position, bool gaps) {
  std::vector<Row> tab(n);
  for (Row& w : tab) {
    size_t len = position + 1 + g_rng.rnd32() % 3;
    if (gaps && g_rng.rnd32() % 7 == 0) len = g_rng.rnd32() % (position + 1);  // lacks the position
    for (size_t e = 0; e < len; ++e) w.elems.push_back(p[g_rng.rnd32() % p.size()]);
    if (gaps) {
      w.col_live = g_rng.rnd32() % 9 != 0;
      w.tab_live = g_rng.rnd32() % 9 != 0;
      w.in_mask = g_rng.rnd32() % 4 != 0;
    }
  }
  return tab;
}

void check_digest(const std::vector<std::string>& p) {
  for (const std::string& s : p) {
    need(strkey_digest(bytes(s), s.size(), 0) == str_digest(bytes(s), s.size()), "salt 0 differs from str_digest");
    for (uint64_t salt = 1; salt < (uint64_t)kStrKeyPasses; ++salt)
      need(strkey_digest(bytes(s), s.size(), salt) != strkey_digest(bytes(s), s.size(), 0),
           "a salt that changes nothing");
  }
  need((kStrKeySalt & 1) == 1, "the salt multiplier is even");
  need(strkey_sort_key(0xF123456789ABCDEFull, 64) == (int64_t)0xF123456789ABCDEFull, "64 bits: the digest itself");
  need(strkey_sort_key(0xF123456789ABCDEFull, 4) == 0xF && strkey_sort_key(0xF123456789ABCDEFull, 1) == 1,
       "the top bits");
  std::printf("ok digest\n");
}

void check_tables(const std::vector<std::string>& p) {
  for (uint64_t position : {0ull, 1ull, 3ull}) {
    for (int gaps = 0; gaps < 2; ++gaps) {
      const std::vector<Row> tab = table(p, 900, position, gaps != 0);
      const Grouping want = reference(tab, position);
      const Grouping got = model(tab, position, 64, false);
      same(got, want, "full digest");
      need(got.passes == 1, "a 64-bit collision among the pool's texts");
      std::printf("ok table position=%llu gaps=%d groups=%zu\n", (unsigned long long)position, gaps, want.first.size());
    }
  }
  // nothing takes part
  std::vector<Row> none = table(p, 50, 0, false);
  for (Row& w : none) w.tab_live = false;
  const Grouping g = model(none, 0, 64, false);
  need(g.ok && g.first.empty() && g.passes == 1, "no participating row");
  std::printf("ok table empty\n");
}

void check_truncated(const std::vector<std::string>& p) {
  for (int bits : {1, 4, 8}) {
    // A and B: two six-byte texts whose salt-0 digests share their top `bits` bits (found by counting up)
    const std::string A = "key000";
    const int64_t ka = strkey_sort_key(strkey_digest(bytes(A), A.size(), 0), bits);
    std::string B;
    for (int i = 1; i < 100000 && B.empty(); ++i) {
      char buf[16];
      std::snprintf(buf, sizeof buf, "k%05d", i);
      if (strkey_sort_key(strkey_digest(bytes(std::string(buf)), 6, 0), bits) == ka) B = buf;
    }
    need(B.size() == 6, "no six-byte text collides with A at " + std::to_string(bits) + " bits");
    // A, B, A, B: one segment of four rows in row order, three adjacent pairs unequal
    std::vector<Row> four(4);
    for (size_t r = 0; r < 4; ++r) four[r].elems = {r % 2 ? B : A};
    const Grouping g4 = model(four, 0, bits, false);
    same(g4, reference(four, 0), "A,B,A,B");
    need(g4.passes == 2, "the interleaved segment was not rejected");
    need(g4.rows.size() == 2 && g4.rows[0] == std::vector<uint32_t>({0, 2}) &&
             g4.rows[1] == std::vector<uint32_t>({1, 3}),
         "A,B,A,B groups");
    // the same pair inside a seeded table with gaps: the first pass must be rejected, the second is exact
    std::vector<std::string> q = p;
    q.push_back(A);
    q.push_back(B);
    std::vector<Row> tab = table(q, 700, 1, true);
    tab[3] = Row{true, true, true, {"x", A}};
    tab[5] = Row{true, true, true, {"x", B}};
    const Grouping got = model(tab, 1, bits, false);
    same(got, reference(tab, 1), "truncated first pass");
    need(got.passes == 2, "a first pass of " + std::to_string(bits) + " bits stood");
    std::printf("ok truncated bits=%d\n", bits);
  }
}

void check_give_up(const std::vector<std::string>& p) {
  const std::vector<Row> tab = table(p, 300, 0, false);
  for (int bits : {1, 4}) {
    const Grouping got = model(tab, 0, bits, true);
    need(!got.ok && got.passes == kStrKeyPasses && got.first.empty() && got.rows.empty(),
         "every pass truncated: a grouping came back");
  }
  // one distinct text cannot collide, however few bits
  std::vector<Row> one(5);
  for (Row& w : one) w.elems = {"same"};
  const Grouping g = model(one, 0, 1, true);
  need(g.ok && g.passes == 1 && g.rows.size() == 1 && g.rows[0].size() == 5, "one text under one bit");
  std::printf("ok give-up\n");
}

}  // namespace

int main() {
  const std::vector<std::string> p = pool();
  check_digest(p);
  check_tables(p);
  check_truncated(p);
  check_give_up(p);
  std::printf("strkey_check: all passed\n");
  return 0;
}
