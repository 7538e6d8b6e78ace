// The carry, borrow and tie paths that end every fold, pair product, scan, grouped fold and batched inverse, replayed
// on the CPU lane by lane (check_lanes.hpp: Mont::step, settle, normalize, Grp::cmp, sub, canon) and word by word
// (check_sos.hpp: Sos::split3, monpro, carries, canon), and compared with bn:: integers.
//
// Without arguments, per lane-group shape of kShapes and kTail the dataflow of k_pairs (product by b, product by R²,
// canon), in plain form and with the first product in QP form (against N~ = N·n0, as k_fold's products run), on seeded
// operands and on the largest ones the preconditions allow under an all-ones modulus; per tree shape the dataflow of
// k_pairs_sos (two monpro, canon) likewise, one monpro on operands of 2^31 N - 1 (what the tree's leaves may reach),
// and canon on k·N - 1, k·N, k·N + 1 for every k it can subtract.
//
// carry_check --paths reads lines "kind S TPI W hexN hexA hexB" (kind: lanes, lanes_qp or sos; sos ignores TPI) and
// prints per line a·b mod N in hex and the path record of the replay (tests/carry_cases.py makes the operands,
// tests/test_carry_check.py and tools/make_carry_fixture.py read the records). No HIP, no device code.
#include <cstring>
#include <iostream>
#include <sstream>

#include "check_lanes.hpp"
#include "check_sos.hpp"

using namespace ddshe;
using namespace ddshe::check;

namespace {

// kShapes and kTail of ddshe_shapes.hpp and DDSHE_TREE_SWITCH of ddshe_tree.hip, repeated here because those files
// include the HIP runtime
struct LaneShape {
  int S, TPI, W;
};
constexpr LaneShape kLaneShapes[] = {{40, 2, 28},   {74, 2, 28},   {76, 2, 28},   {112, 4, 28},  {148, 4, 28},
                                     {232, 8, 27},  {320, 16, 27}, {640, 32, 27}, {48, 16, 28},  {80, 16, 28},
                                     {112, 16, 28}, {160, 16, 28}, {240, 16, 27}};
struct TreeShape {
  int S, W;
};
constexpr TreeShape kTreeShapes[] = {{46, 26}, {84, 26}, {86, 26}, {124, 26}, {162, 26}, {244, 26}, {336, 26}, {694, 25}};

std::string tag(const LaneShape& s, bool qp) {
  return "(" + std::to_string(s.S) + ", " + std::to_string(s.TPI) + ", " + std::to_string(s.W) + ")" +
         (qp ? " QP" : " plain");
}

void lane_shape(const LaneShape& s, bool qp) {
  const std::string id = tag(s, qp);
  // the widest modulus of the form: R > 4N, and R > 4N~ (N~ < 2^W N) in QP form
  const size_t bits = (size_t)s.W * s.S - 2 - (qp ? s.W : 0);
  {
    const bn::Limbs N = lcg_odd(bits, 0xca11u + s.S * 64 + s.TPI + (qp ? 1 : 0));
    Lcg g{0x5eedu + (uint64_t)s.S};
    for (int i = 0; i < 3; ++i) {
      const bn::Limbs a = g.rnd_below(N), b = g.rnd_below(N);
      LanePaths p;
      need(bn::cmp(lane_pair(s.S, s.TPI, s.W, qp, N, a, b, &p, id + " seeded"), bn::mulmod(a, b, N)) == 0,
           id + " seeded: not a b mod N");
    }
  }
  {
    // all-ones modulus; a column row may be anything below 2N
    const bn::Limbs N = pow2m1(bits), top = bn::sub(bn::add(N, N), bn::Limbs{1});
    LanePaths p;
    need(bn::cmp(lane_pair(s.S, s.TPI, s.W, qp, N, top, top, &p, id + " capacity"), bn::mulmod(top, top, N)) == 0,
         id + " capacity: not a b mod N");
  }
  std::printf("ok lanes %s\n", id.c_str());
}

void tree_shape(const TreeShape& s) {
  const std::string id = "(" + std::to_string(s.S) + ", " + std::to_string(s.W) + ")";
  const size_t bits = (size_t)s.W * s.S - 64;  // R >= 2^64 N
  {
    const bn::Limbs N = lcg_odd(bits, 0x7eeu + s.S);
    Lcg g{0x5eedu + (uint64_t)s.S};
    for (int i = 0; i < 3; ++i) {
      const bn::Limbs a = g.rnd_below(N), b = g.rnd_below(N);
      SosPaths p;
      need(bn::cmp(sos_pair(s.S, s.W, N, a, b, &p, id + " seeded"), bn::mulmod(a, b, N)) == 0,
           id + " seeded: not a b mod N");
    }
  }
  const bn::Limbs N = pow2m1(bits);
  {
    const bn::Limbs top = bn::sub(N, bn::Limbs{1});
    SosPaths p;
    need(bn::cmp(sos_pair(s.S, s.W, N, top, top, &p, id + " capacity"), bn::mulmod(top, top, N)) == 0,
         id + " capacity: not a b mod N");
  }
  SosSim sim(s.S, s.W, N, id + " leaves");
  {
    // one product of the largest leaves the tree allows (below 2^31 N): monpro checks its own bounds
    const bn::Limbs leaf = bn::sub(bn::mul(bn::pow2(31), N), bn::Limbs{1});
    std::vector<uint32_t> a = bn::to_rw(leaf, s.S, s.W);
    sim.monpro(a, bn::to_rw(leaf, s.S, s.W));
    SosPaths p;
    sim.canon(a, &p);
  }
  // canon at every multiple it can subtract, and one below and above each
  bn::Limbs kN;
  for (int k = 0; k <= 4; ++k) {
    for (int d = -1; d <= 1; ++d) {
      if ((k == 0 && d < 0) || (k == 4 && d >= 0)) continue;
      const bn::Limbs u = d < 0 ? bn::sub(kN, bn::Limbs{1}) : d > 0 ? bn::add(kN, bn::Limbs{1}) : kN;
      std::vector<uint32_t> a = bn::to_rw(u, s.S, s.W);
      SosPaths p;
      sim.canon(a, &p);
      need(p.k == (d < 0 ? k - 1 : k), id + " canon: subtracted another multiple than expected");
    }
    kN = bn::add(kN, N);
  }
  std::printf("ok sos %s\n", id.c_str());
}

int paths() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string kind, hn, ha, hb;
    int S = 0, TPI = 0, W = 0;
    in >> kind >> S >> TPI >> W >> hn >> ha >> hb;
    need(!in.fail(), "--paths: a line is not 'kind S TPI W hexN hexA hexB'");
    const bn::Limbs N = from_hex(hn.c_str()), A = from_hex(ha.c_str()), B = from_hex(hb.c_str());
    if (kind == "lanes" || kind == "lanes_qp") {
      LanePaths p;
      const bn::Limbs r = lane_pair(S, TPI, W, kind == "lanes_qp", N, A, B, &p, kind);
      std::printf("%s rounds=%d ties=%d cmp=%d sub=%d hops=%d\n", to_hex(r).c_str(), p.rounds, p.tie_lanes, p.cmp,
                  p.sub ? 1 : 0, p.borrow_hops);
    } else if (kind == "sos") {
      SosPaths p;
      const bn::Limbs r = sos_pair(S, W, N, A, B, &p, kind);
      std::printf("%s prop=%d run=%d cross=%d k=%d ncmp=%d", to_hex(r).c_str(), p.prop_bits, p.carry_run,
                  p.carry_cross ? 1 : 0, p.k, p.ncmp);
      for (int i = 0; i < p.ncmp; ++i) std::printf(" tie%d=%d tiex%d=%d", i, p.tie[i], i, p.tie_cross[i] ? 1 : 0);
      std::printf("\n");
    } else {
      die("--paths: unknown kind " + kind);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--paths") == 0) return paths();
  for (const LaneShape& s : kLaneShapes)
    for (int qp = 0; qp < 2; ++qp) lane_shape(s, qp != 0);
  for (const TreeShape& s : kTreeShapes) tree_shape(s);
  std::printf("carry_check: all passed\n");
  return 0;
}
