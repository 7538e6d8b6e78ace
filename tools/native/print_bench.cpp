// The host route to the store's text that dds_col_read_dec replaces: BigInteger.toString of every row of a
// big-endian buffer (what dds_col_read returns) with the engine's own bn::to_dec, on one core.
//   print_bench <rows.bin> <width> <rows> <out.txt>
// reads rows * width bytes, prints the rows back to back into out.txt (no separators, the layout of
// dds_col_read_dec's chars) and reports one JSON line: seconds spent printing (file I/O excluded).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bn_host.hpp"

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: print_bench <rows.bin> <width> <rows> <out.txt>\n");
    return 2;
  }
  const size_t width = std::strtoull(argv[2], nullptr, 10), rows = std::strtoull(argv[3], nullptr, 10);
  std::vector<uint8_t> in(width * rows);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), 1, in.size(), f) != in.size()) {
    std::fprintf(stderr, "print_bench: cannot read %zu bytes from %s\n", in.size(), argv[1]);
    return 1;
  }
  std::fclose(f);
  std::string out;
  out.reserve(rows * (width * 5 / 2 + 1));
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < rows; ++i) out += ddshe::bn::to_dec(ddshe::bn::from_be(in.data() + i * width, width));
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  f = std::fopen(argv[4], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "print_bench: cannot write %s\n", argv[4]);
    return 1;
  }
  std::printf("{\"rows\": %zu, \"chars\": %zu, \"print_s\": %.6f}\n", rows, out.size(), s);
  return 0;
}
