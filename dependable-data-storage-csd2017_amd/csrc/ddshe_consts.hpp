// The numbers that kernels, host code and the CPU check programs all need, defined once. No HIP: the check
// programs (*_check.cpp) and the plan headers include it alone; ddshe_launch.hpp and ddshe_ladder1.hpp
// include it for everything else.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace ddshe {

// per-modulus constant block: 5 vectors of S r27 limbs each
enum { kConstN = 0, kConstRmod = 1, kConstR2 = 2, kConstOne = 3, kConstN2x = 4, kConstCount = 5 };

// Digit-form fold of a perfect-square modulus n² in the (148, 4, 28) shape (ddshe_foldsq.hpp): values as
// two base-n digits of kFoldSqLimbs limbs each. sq: kSqCount vectors of kFoldSqLimbs limbs (ñ = k·n | n |
// C | R mod n | R² mod n), k = -n⁻¹ mod 2^28.
constexpr int kFoldSqLimbs = 76, kFoldSqWide = 148;
enum { kSqNq = 0, kSqN = 1, kSqC = 2, kSqRmod = 3, kSqR2 = 4, kSqCount = 5 };  // kSqR2: R² mod n

// Unit form of the mirror (ddshe_foldunit.hpp), and the batch inversion it shares with the row-wise inverses
// (ddshe_inv_plan.hpp).
// rows per group of one inversion level, and the row count at or below which the host finishes
constexpr size_t kInvFan = 32;
// rows whose prefix products one pass holds in scratch (kFoldSqLimbs limbs each for the mirror's upgrade, S limbs
// for the row-wise calls, which take fewer where that plane would exceed 1 GiB: inv_chunk_rows)
constexpr size_t kInvChunkRows = (size_t)1 << 20;
// rows per group k_fold_unit admits: the sum of the b stays below R
constexpr size_t kFoldUnitMaxRowsPerGroup = (size_t)1 << 26;
// rows added to the 32-bit limbs of the sum of the b between two carry passes (MontUnit::kSumRows)
constexpr int kFoldUnitSumRows = 8;
// rows per lane pair from which a fold takes the kernel at one chain per lane (ddshe_foldunit1.hpp,
// fold_unit1_min_rows)
constexpr size_t kFoldUnit1RowsPerPair = 16;

// constant block of the one-bignum-per-lane ladder (ddshe_ladder1.hpp, built by host::ladder1_consts):
// kL1Count vectors of S1 limbs
enum { kL1Mod = 0, kL1N = 1, kL1Rmod = 2, kL1R2 = 3, kL1Count = 4 };

}  // namespace ddshe
