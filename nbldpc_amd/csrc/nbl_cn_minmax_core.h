// nbldpc_amd/csrc/nbl_cn_minmax_core.h -- the Min-Max check-node programme (method 3; nbl_create_minmax; kernels in nbl_cn_minmax.hip,
// flooding and layered), one instantiation per q for every check degree 2 .. NBL_MINMAX_MAX_CHECK_DEGREE.
//
// The update is the one include/nbldpc.h defines: check domain, dissimilarities u_d[y] = m_d - p_d[y] (one rounded subtraction), the
// combination w_d[y] = min over the configurations of the other edges with XOR y of the max of their dissimilarities, back to LLRs
// c_d[y] = w_d[0] - w_d[y] (one rounded subtraction), shaping, un-permuting.  Between the two subtractions there is nothing but v_min_f64
// and v_max_f64 on finite non-negative doubles: both select one of their operands and never round, so the forward / backward recursion
// with the elementary step E(A,B)[c] = min_a max(A[a], B[a ^ c]) gives the minimum over the configuration SET whatever order the terms
// are taken in (max(min_i x_i, b) = min_i max(x_i, b)).  E is symmetric in its operands (substitute a -> a ^ c).
//
// Layout: the storage scheme of nbl_cn_bp_wide_core.h.
//
//   one check per WORKGROUP of W = max(1, Q / 64) waves.  Wave w stages edges w, w + W, ..: the edge's maximum is one wave reduction (a
//   wave holds a whole vector), the dissimilarities go into U[d] at their check-domain slots.  A WORKGROUP barrier follows.  From there
//   on thread s owns symbol s alone (Q < 64: the lanes below Q).
//
//   an elementary step reads one operand at the workgroup-uniform index x (a broadcast read) and one at s ^ x.  x runs in pairs: the
//   16-byte read at pair (s >> 1) ^ (x >> 1) holds B[s ^ x] and B[s ^ x ^ 1], in that order for an even s and swapped for an odd one, so
//   an odd thread swaps the uniform pair instead -- a term is max(A[x], B[s ^ x]) either way, and the order of the terms is immaterial.
//   The uniform operand of a step is U[k], already in LDS; the running partial goes from its owner's register into one [Q] block.
//
//   F_d (d >= 1) is parked in the check's own c2v region C[d] until that region's final store: thread s writes slot s, reads back slot s
//   and later stores the final entry s over it -- program order of one thread at one address is all the ordering this needs.  The
//   outputs are produced from the last edge down while the running R advances in a register per thread; the middle output E(F_d, R_d)
//   and the advance E(u_d, R_d) share the XOR-addressed reads of R_d in one loop.
//
// LDS: [maxdc][Q] dissimilarities, two [Q] operand blocks, two [Q] output vectors: (maxdc + 4) q 8 bytes (nbl_minmax_lds_bytes), 73,728 B
// at q = 256 and degree 32 -- below the 160 KB of a workgroup for every shape the ABI accepts; above 64 KB the launcher opts in.
//
// Barriers.  Forward step k writes block k & 1, one barrier, reads it; block k & 1 was last read by step k - 2, which every thread left
// before the barrier of step k - 1.  Output d writes both blocks (middle outputs only), one barrier, reads them, writes output vector
// d & 1, one barrier, reads it; the blocks' readers of output d are done before that second barrier, and vector d & 1 was last read by
// output d + 2, before the second barrier of output d + 1.  Every barrier is in workgroup-uniform control flow: dc and the loop
// counters are uniform; the caller's early returns are per workgroup.
//
// Aliasing (the layered schedule): as in nbl_cn_bp_wide_core.h.  input() of every wave reads C and the c2v of the neighbours; the first
// write into C is the F_1 store, behind the workgroup barrier that follows the staging loop.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"

template <int Q> struct MinMax {
	static constexpr int W = Q >= 64 ? Q / 64 : 1; // waves of a check's workgroup
	static constexpr int NT = 64 * W;
};

struct NblMmPair { double x, y; };

// min over x of max(A[x], B[sb ^ x]); A, B: [Q] in LDS, 16-byte aligned
template <int Q> __device__ __forceinline__ double minmax_step(const double *A, const double *B, int sb)
{
	const NblMmPair *A2 = (const NblMmPair *)A, *B2 = (const NblMmPair *)B;
	const bool odd = sb & 1;
	const int h = sb >> 1;
	double acc = __builtin_huge_val();
#pragma unroll 4
	for (int x2 = 0; x2 < Q / 2; x2++) {
		const NblMmPair a = A2[x2], b = B2[h ^ x2];
		acc = dmin(acc, dmax(odd ? a.y : a.x, b.x));
		acc = dmin(acc, dmax(odd ? a.x : a.y, b.y));
	}
	return acc;
}

// the same for two uniform operands against one XOR-addressed operand: o1 = E(A1, B)[sb], o2 = E(A2, B)[sb]
template <int Q> __device__ __forceinline__ void minmax_step2(const double *A1, const double *A2, const double *B, int sb, double &o1, double &o2)
{
	const NblMmPair *P1 = (const NblMmPair *)A1, *P2 = (const NblMmPair *)A2, *B2 = (const NblMmPair *)B;
	const bool odd = sb & 1;
	const int h = sb >> 1;
	double acc1 = __builtin_huge_val(), acc2 = __builtin_huge_val();
#pragma unroll 4
	for (int x2 = 0; x2 < Q / 2; x2++) {
		const NblMmPair a1 = P1[x2], a2 = P2[x2], b = B2[h ^ x2];
		acc1 = dmin(acc1, dmax(odd ? a1.y : a1.x, b.x));
		acc1 = dmin(acc1, dmax(odd ? a1.x : a1.y, b.y));
		acc2 = dmin(acc2, dmax(odd ? a2.y : a2.x, b.x));
		acc2 = dmin(acc2, dmax(odd ? a2.x : a2.y, b.y));
	}
	o1 = acc1;
	o2 = acc2;
}

// One check of `dc` edges starting at check-major edge c0, by the calling workgroup of MinMax<Q>::NT threads; `smem` is its dynamic LDS
// (nbl_minmax_lds_bytes).  input(j) returns a callable a -> entry a of the input of edge j (a = 1 .. Q-1); it is called by ONE wave per
// edge (wave j % W) and only before the first workgroup barrier.  C: the check's c2v region [dc][Q]; it may alias what input() reads.
template <int Q, class Input>
__device__ __forceinline__ void minmax_check_node(const NblGraphDev &g, const NblRun &r, char *smem, int c0, int dc, double *C, Input input)
{
	constexpr int NS = Fld<Q>::NS, W = MinMax<Q>::W;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

	double *U = (double *)smem;      // [maxdc][Q] dissimilarities in the check domain: U[d][h_d a] = m_d - in_d[a], U[d][0] = m_d
	double *P0 = U + g.maxdc * Q;    // [Q] operand block (forward: partial of an even step; outputs: F_d)
	double *P1 = P0 + Q;             // [Q] operand block (forward: partial of an odd step; outputs: R_d)
	double *T = P1 + Q;              // [2][Q] w_d before its permutation, output d in vector d & 1

	for (int d = wave; d < dc; d += W) {
		const auto vd = input(d);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
		double v[NS];
		double best = 0.0; // (slot 0 holds 0: the maximum includes it)
#pragma unroll
		for (int i = 0; i < NS; i++) {
			const int a = lane + 64 * i;
			v[i] = (a < Q && a > 0) ? vd(a) : 0.0;
			best = dmax(best, v[i]);
		}
		const double m = wave_fmax_nonneg(best);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			const int a = lane + 64 * i;
			if (a < Q) U[d * Q + mh.at_slot(i)] = m - v[i];
		}
	}
	__syncthreads(); // every input() of every wave is complete: C is free from here on

	const int s = tid;
	const bool own = Q >= 64 || s < Q;
	const int sb = own ? s : 0; // (a thread without a symbol computes on symbol 0's addresses and stores nothing)
	// forward partials: F_1 = u_0, F_{k+1} = E(F_k, u_k); F_k parked in C[k][s]
	double f = U[sb];
#pragma unroll 1
	for (int k = 1; k + 1 <= dc - 1; k++) {
		double *Pk = (k & 1) ? P1 : P0;
		if (own) {
			C[(size_t)k * Q + s] = f;
			Pk[s] = f;
		}
		__syncthreads();
		f = minmax_step<Q>(U + k * Q, Pk, sb);
	}
	// from the last edge down: rr = R_d, R_{dc-2} = u_{dc-1}, R_{d-1} = E(R_d, u_d)
	double rr = U[(dc - 1) * Q + sb];
#pragma unroll 1
	for (int d = dc - 1; d >= 0; d--) {
		double *Cd = C + (size_t)d * Q;
		double *Td = T + (d & 1) * Q;
		double val, rnext = rr;
		if (d == dc - 1) val = f;  // F_{dc-1}
		else if (d == 0) val = rr; // R_0
		else {
			if (own) {
				P0[s] = Cd[s]; // F_d, this thread's own store
				P1[s] = rr;
			}
			__syncthreads();
			minmax_step2<Q>(P0, U + d * Q, P1, sb, val, rnext);
		}
		if (own) Td[s] = val;
		__syncthreads();
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
		if (own) Cd[s] = (s == 0) ? 0.0 : shape_llr(Td[0] - Td[mh.at_slot(wave)], r.factor, r.offset);
		rr = rnext;
	}
}
