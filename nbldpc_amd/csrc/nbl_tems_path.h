// nbldpc_amd/csrc/nbl_tems_path.h -- the path code of the wide T-EMS programme (nbl_cn_tems_wide_core.h): the winning trellis path of a
// check sum in a word that does not grow with the check degree.  Plain C++, host and device: the kernels and the host export
// nbl_debug_tems_wide_path_key (tests/test_tems_wide.py) run the same lines.
//
// A path is a digit string (q_0 .. q_dc-1), q_d the deviation symbol of column d, 0 = no deviation; the reference keeps the FIRST minimal
// path in enumeration order, which is lexicographic in that string with column 0 most significant (nbl_cn_tems_core.h).  A path has at most
// nc non-zero digits, so only those are stored: the deviations in ascending column order fill slots 0, 1, ..; slot i holds the 13-bit key
// ((31 - col) << 8) | sym with sym >= 1, slot 0 most significant, unused slots 0.
//
// Order: unsigned comparison of two codes = lexicographic comparison of the digit strings.  Take the first slot i in which they differ;
// the slots before it name the same deviations, and neither string has another non-zero digit before the earlier of the two slot-i
// columns.  (a) Same column, different symbols: the strings first differ there and the symbols compare like the keys.  (b) Columns c < c':
// at column c one string has a non-zero digit, the other (whose next deviation is at c' > c) has 0, so the first is the larger string --
// and 31 - c > 31 - c' makes its key the larger.  (c) One slot empty: as (b) with the other string 0 from there on; the key of a
// deviation is never 0 (sym >= 1), so it is larger than the empty slot.  Equal codes name the same deviations: equal strings.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NBL_PATH_HD __host__ __device__ inline
#else
#define NBL_PATH_HD inline
#endif

#define NBL_TEMS_WIDE_MAX_NC 4     // slots of one 64-bit word (4 x 13 = 52 bits)
#define NBL_TEMS_PATH_SLOT_BITS 13 // 5 bits of column (check degrees up to 32), 8 bits of symbol (fields up to GF(256))

// the key of a deviation to symbol `sym` (1 .. 255) in column `col` (0 .. 31)
NBL_PATH_HD uint64_t nbl_tems_path_key(int col, int sym) { return (uint64_t)(((31 - col) << 8) | sym); }

// bit position of the l-th deviation of a path (l = 1 .. NBL_TEMS_WIDE_MAX_NC)
NBL_PATH_HD int nbl_tems_path_shift(int l) { return NBL_TEMS_PATH_SLOT_BITS * (NBL_TEMS_WIDE_MAX_NC - l); }

// `code` holds l - 1 deviations, all in columns before `col`: the code with (col, sym) appended as the l-th.  "No deviation in this
// column" leaves a code unchanged.
NBL_PATH_HD uint64_t nbl_tems_path_append(uint64_t code, int l, int col, int sym) { return code | (nbl_tems_path_key(col, sym) << nbl_tems_path_shift(l)); }

// a comes before b in enumeration order
NBL_PATH_HD bool nbl_tems_path_before(uint64_t a, uint64_t b) { return a < b; }

// the digit of column `col`: the symbol of the slot whose column it is, else 0 (an empty slot reads as column 31 with symbol 0)
NBL_PATH_HD int nbl_tems_path_digit(uint64_t code, int col)
{
	int sym = 0;
	for (int l = 1; l <= NBL_TEMS_WIDE_MAX_NC; l++) {
		const unsigned slot = (unsigned)(code >> nbl_tems_path_shift(l)) & ((1u << NBL_TEMS_PATH_SLOT_BITS) - 1u);
		if ((int)(slot >> 8) == 31 - col) sym |= (int)(slot & 255u);
	}
	return sym;
}
