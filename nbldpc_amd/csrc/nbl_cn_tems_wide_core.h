// nbldpc_amd/csrc/nbl_cn_tems_wide_core.h -- the trellis-EMS check-node programme for checks of degree up to NBL_TEMS_MAX_CHECK_DEGREE and
// any field (nbl_create_tems_wide; kernels in nbl_cn_tems_wide.hip, flooding and layered).  The arithmetic is tems_check_node's
// (nbl_cn_tems_core.h) operation for operation: beta, syndrome and dU; the stable column order and its nr marks; the min-plus DP over
// the columns with one layer per deviation count, left-to-right sums, smallest (cost, path in enumeration order) per check sum; the
// scatter with fetch_min, the fill from the first two columns of the order, shape_llr.  So the result is the same bit for bit
// (tests/test_gpu_tems_wide.py holds the two to that).  What differs is the layout, in which nothing is sized by the degree:
//
//   path code.  tems_check_node keeps the path of a check sum as dc base-q digits in 32 bits.  Here it is the 64-bit word of
//   nbl_tems_path.h -- the at most nc <= NBL_TEMS_WIDE_MAX_NC deviations as (column, symbol) keys -- which orders like the digit string.
//
//   one check per WORKGROUP of W = max(1, Q / 64) waves (TemsWide<Q>).  Wave w stages edges w, w + W, .. (step 1 is per edge); a workgroup
//   barrier follows, so every input is read before the first output is written and C may alias what input() reads -- tems_check_node's
//   contract, now across waves.  From step 2 on thread t owns symbol t alone (Q < 64: the lanes below Q).
//
//   column order.  Only the nr smallest columns of the stable order (dU, column), its first and its second column are read afterwards:
//   they are selected in max(2, min(nr, dc)) passes over the columns, each taking the smallest column after the one taken before it --
//   exactly the ranks 0, 1, .. of the full sort, dc nr compares per symbol instead of dc^2.  The mark set is an unsigned word.
//
//   candidate lists.  Per-column offsets plus one array of at most min(nr, maxdc) (q - 1) packed {dU, symbol} entries, read as LDS
//   broadcasts; counted, offset, filled.  The order of a list's entries is not defined (as in tems_check_node) and does not matter:
//   (cost, path code) is a total order on paths.
//
// Every edge, column and layer loop is a run-time loop: one instantiation per q serves every degree.  Every barrier is in
// workgroup-uniform control flow (dc, nr, nc and the list bounds are uniform; the caller's early returns are per workgroup).
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_tems_path.h"

template <int Q> struct TemsWide {
	static constexpr int W = Q >= 64 ? Q / 64 : 1; // waves of a check's workgroup
	static constexpr int NT = 64 * W;
};

struct __attribute__((aligned(16))) TWState { double v; unsigned long long c; }; // cost and path code of one (layer, check sum)
struct __attribute__((aligned(16))) TWCand { double u; int q; int pad; };         // one allowed deviation of a column: dU and symbol

// LDS of one check, in bytes (host arithmetic; nbl_tems_wide_lds_bytes of nbl_cn_tems_wide.hip is this function): dU [maxdc][q] and Lc [q]
// doubles, the DP states [2][nc + 1][q], the candidate array, ord01 [q], the column offsets, cursors and beta
inline size_t nbl_tems_wide_lds_layout(size_t q, size_t maxdc, size_t nr, size_t nc)
{
	const size_t cand = (nr < maxdc ? nr : maxdc) * (q - 1);
	return (maxdc * q + q) * 8 + 2 * (nc + 1) * q * sizeof(TWState) + cand * sizeof(TWCand) + q * 4 + (3 * maxdc + 4) * 4;
}

// One check of `dc` edges starting at check-major edge c0, by the calling workgroup of TemsWide<Q>::NT threads; `smem` is its dynamic
// LDS (nbl_tems_wide_lds_bytes).  input(d, v) and C as for tems_check_node; input() is called by one whole wave per edge.
template <int Q, class Input>
__device__ __forceinline__ void tems_wide_check_node(const NblGraphDev &g, const NblRun &r, char *smem, int c0, int dc, double *C, Input input)
{
	constexpr int NS = Fld<Q>::NS, W = TemsWide<Q>::W, NT = TemsWide<Q>::NT, NL = NBL_TEMS_WIDE_MAX_NC + 1;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int nc = r.nc, layers = nc + 1, mdc = g.maxdc;
	const int nsel = r.nr < dc ? r.nr : dc; // marked columns per symbol

	double *dU = (double *)smem;                       // [mdc][Q]
	double *Lc = dU + mdc * Q;                         // [Q]
	TWState *st = (TWState *)(Lc + Q);                 // [2][layers][Q] DP states (ping-pong)
	TWCand *cl = (TWCand *)(st + 2 * layers * Q);      // [min(nr, mdc) (Q - 1)] deviation candidates, column after column
	int *ord01 = (int *)(cl + (r.nr < mdc ? r.nr : mdc) * (Q - 1)); // [Q] first two columns of the per-symbol order (lo byte, next byte)
	int *coff = ord01 + Q;                             // [mdc + 1] list of column d: cl[coff[d]] .. cl[coff[d + 1] - 1]
	int *ccount = coff + mdc + 1;                      // [mdc] entries of column d, then the fill cursor
	int *beta = ccount + mdc;                          // [mdc]

	// ---- 1. beta, dU: wave w takes edges w, w + W, .. (tems_stage_inputs, per edge) ---------------------------------------------------
	for (int d = wave; d < dc; d += W) {
		double v[NS];
		input(d, v);
		// most reliable symbol: strict '>' over ascending symbols from a running maximum of 0
		double best = 0.0;
		int arg = 0;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q && v[i] > best) { best = v[i]; arg = a; }
		}
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			double ob = __shfl_xor(best, off, 64);
			int oa = __shfl_xor(arg, off, 64);
			if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
		}
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
		// beta_d = h * argmax (0 if nothing positive)
		int bd = 0;
		{
			int x = g.c_h[c0 + d];
			for (int k = 0; k < 8; k++) {
				if ((arg >> k) & 1) bd ^= x;
				x <<= 1;
				if (x & Q) x ^= g.poly;
			}
		}
		bd = uniform(bd);
		const double mx = uniform_f64(best); // = L(argmax), or 0 when beta = 0
		if (lane == 0) beta[d] = bd;
		// dU[d][h a ^ beta] = mx - L(a), L(0) = 0
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) dU[d * Q + (mh.at_slot(i) ^ bd)] = mx - v[i];
		}
	}
	for (int d = tid; d < dc; d += NT) ccount[d] = 0;
	__syncthreads();
	int syn = 0;
	for (int d = 0; d < dc; d++) syn ^= beta[d];

	const int s = tid;                 // the check sum / deviation symbol this thread owns
	const bool own = Q >= 64 || s < Q;

	// ---- 2. per deviation symbol: the first columns of the stable ascending order (dU, column); the nr smallest marked ----------------
	unsigned mask = 0;
	if (own) {
		double pu = 0.0;
		int pd = -1, o0 = 0, o1 = 0;
		const int rounds = nsel > 2 ? nsel : 2; // (dc >= 2)
		for (int k = 0; k < rounds; k++) {
			// the smallest (u, d) after (pu, pd); ascending d with a strict '<' keeps the lowest column among equals
			double bu = 0.0;
			int bd = -1;
			for (int d = 0; d < dc; d++) {
				const double u = dU[d * Q + s];
				const bool after = pd < 0 || u > pu || (u == pu && d > pd);
				if (after && (bd < 0 || u < bu)) { bu = u; bd = d; }
			}
			if (bd < 0) break; // (only with NaN inputs: no column compares)
			if (k < nsel) mask |= 1u << bd;
			if (k == 0) o0 = bd;
			if (k == 1) o1 = bd;
			pu = bu;
			pd = bd;
		}
		ord01[s] = o0 | (o1 << 8);
		// candidate lists hold non-zero symbols only; symbol 0 = "no deviation" is handled apart (its mark set, every column, is never read)
		if (s == 0) mask = 0;
		for (int d = 0; d < dc; d++)
			if ((mask >> d) & 1u) atomicAdd(&ccount[d], 1);
	}
	__syncthreads();
	if (tid == 0) {
		int acc = 0;
		for (int d = 0; d < dc; d++) {
			const int n = ccount[d];
			coff[d] = acc;
			ccount[d] = acc; // the fill cursor
			acc += n;
		}
		coff[dc] = acc;
	}
	__syncthreads();
	if (own) {
		for (int d = 0; d < dc; d++)
			if ((mask >> d) & 1u) {
				TWCand e;
				e.u = dU[d * Q + s];
				e.q = s;
				e.pad = 0;
				cl[atomicAdd(&ccount[d], 1)] = e;
			}
	}

	// ---- 3. min-plus DP over the columns; all deviation-count layers advance together ----------------------------------------------
	// state of (layer l, check sum s): cost and path code of the best path with exactly l deviating columns
	TWState *A = st, *B = st + layers * Q;
	for (int idx = tid; idx < layers * Q; idx += NT) {
		TWState z;
		z.v = (idx == 0) ? 0.0 : __builtin_huge_val();
		z.c = 0;
		A[idx] = z;
	}
	__syncthreads();
	for (int d = 0; d < dc; d++) {
		const int k0 = coff[d], k1 = coff[d + 1];
		TWState b[NL];
#pragma unroll
		for (int l = 0; l < NL; l++) {
			if (own && l <= nc) {
				b[l] = A[l * Q + s]; // q_d = 0: dU[d][0] = 0, the code is unchanged
				b[l].v = b[l].v + 0.0;
			}
		}
		for (int k = k0; k < k1; k++) {
			const TWCand e = cl[k]; // LDS broadcast
			const unsigned long long key = nbl_tems_path_key(d, e.q);
			if (own) {
#pragma unroll
				for (int l = 1; l < NL; l++) {
					if (l <= nc && l <= d + 1) { // a path through d + 1 columns has at most d + 1 deviations
						const TWState src = A[(l - 1) * Q + (s ^ e.q)];
						const double val = src.v + e.u;
						const unsigned long long code = src.c | (key << nbl_tems_path_shift(l));
						// smaller cost wins, equal cost: the path that comes first in enumeration order
						if (val < b[l].v || (val == b[l].v && nbl_tems_path_before(code, b[l].c))) { b[l].v = val; b[l].c = code; }
					}
				}
			}
		}
#pragma unroll
		for (int l = 0; l < NL; l++)
			if (own && l <= nc) B[l * Q + s] = b[l];
		__syncthreads();
		TWState *t = A; A = B; B = t;
	}
	// dW, Eta: best layer per check sum
	double dW = __builtin_huge_val();
	unsigned long long eta = ~0ull;
	if (own) {
#pragma unroll
		for (int l = 0; l < NL; l++) {
			if (l <= nc) {
				const TWState f = A[l * Q + s];
				if (f.v < dW || (f.v == dW && nbl_tems_path_before(f.c, eta))) { dW = f.v; eta = f.c; }
			}
		}
	}

	// ---- 4. outputs (tems_outputs, one symbol per thread) -----------------------------------------------------------------------------
	for (int d = 0; d < dc; d++) {
		__syncthreads();
		if (own) Lc[s] = NBL_DBL_MAX;
		__syncthreads();
		if (own) {
			const int dev = nbl_tems_path_digit(eta, d);
			const double cand = dW - dU[d * Q + dev];
			__hip_atomic_fetch_min(&Lc[s ^ dev], cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		}
		__syncthreads();
		if (own && Lc[s] == NBL_DBL_MAX) { // never reached
			const int o0 = ord01[s] & 255, o1 = (ord01[s] >> 8) & 255;
			Lc[s] = (d == o0) ? dU[o1 * Q + s] : dU[o0 * Q + s];
		}
		__syncthreads();
		// delta domain -> LLR, un-permute by h
		const int bsyn = syn ^ beta[d];
		const double L0 = -1.0 * Lc[bsyn];
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
		if (own) {
			const int e = mh.at_slot(wave) ^ bsyn; // eta with h^-1 (eta ^ bsyn) = s
			C[(size_t)d * Q + s] = (s == 0) ? 0.0 : shape_llr(-1.0 * Lc[e] - L0, r.factor, r.offset);
		}
	}
}
