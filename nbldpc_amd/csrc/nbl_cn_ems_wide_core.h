// nbldpc_amd/csrc/nbl_cn_ems_wide_core.h -- the EMS check-node programme for checks of degree up to NBL_EMS_MAX_CHECK_DEGREE
// (nbl_create_ems_wide; kernels in nbl_cn_ems_wide.hip, flooding and layered).  The arithmetic is ems_check_node's
// (nbl_cn_ems_core.h) operation for operation: the same configuration set, the same left-to-right sums ((0.0 + x1) + x2) + .. per output
// edge, so the result is the same bit for bit (tests/test_gpu_ems_wide.py holds the two to that).  What differs is who does what:
//
//   one check per WORKGROUP of W = max(1, Q / 64) waves.  Wave w stages edges w, w + W, .. (permutation into the check domain and the
//   top-nm selection are per edge and independent between edges); a workgroup barrier follows, so every input is read before the first
//   output is written and C may alias what input() reads -- ems_check_node's contract, now across waves.  In the output phase thread
//   t owns symbol t alone (Q < 64: the lanes below Q), so the XOR gathers A[sym ^ t] spread over the waves.
//
//   shared prefix.  The DP state over edges 0 .. x-1 is the same for every output edge x: it lives in LDS as P.  Output x continues
//   from P over edges x+1 .. dc-1 (ping, pong), then P advances by edge x: about dc (dc + 1) / 2 steps per check instead of dc (dc - 1).
//   conf(q,1) the same way: the sum of the rank-0 values left of the deviating edge is one running scalar; only the adds to its right
//   are per symbol.
//
// No array is sized by the degree and every edge loop is a run-time loop: one instantiation per q serves every degree.  Every barrier
// is in workgroup-uniform control flow (dc, x, the layer count and nc are uniform; the caller's early returns are per workgroup).
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_cn_ems_core.h" // select_top

template <int Q> struct EmsWide {
	static constexpr int W = Q >= 64 ? Q / 64 : 1; // waves of a check's workgroup
	static constexpr int NT = 64 * W;
};

// One DP step over edge j (lists lvj / ltj, rank 0 first): dst = src (*) edge j.  layers > 1: layer d counts deviations, rank 0 keeps
// the layer and ranks 1 .. nm-1 come from the layer below; layers == 1 (nc >= maxdc - 1): the plain truncated max-plus convolution.
// Reads src, writes dst[.][sym] only: the caller puts a barrier between a step and whatever reads dst or rewrites src.
template <int Q>
__device__ __forceinline__ void ems_wide_step(const double *src, double *dst, const double *lvj, const int *ltj, int nm, int layers, int sym, bool own)
{
	const int z = ltj[0];
	const double mz = lvj[0];
	for (int d = 0; d < layers; d++) {
		double acc = own ? src[d * Q + (sym ^ z)] + mz : NBL_NEG_INF;
		if (d >= 1 || layers == 1) {
			const double *from = src + (layers == 1 ? 0 : (d - 1) * Q);
			for (int k = 1; k < nm; k++) {
				const int tk = uniform(ltj[k]);
				const double vk = lvj[k];
				if (own) acc = dmax(acc, from[sym ^ tk] + vk);
			}
		}
		if (own) dst[d * Q + sym] = acc;
	}
}

// One check of `dc` edges starting at check-major edge c0, by the calling workgroup of EmsWide<Q>::NT threads; `smem` is its dynamic
// LDS (nbl_ems_wide_lds_bytes).  input(j) and C as for ems_check_node.
template <int Q, class Input>
__device__ __forceinline__ void ems_wide_check_node(const NblGraphDev &g, const NblRun &r, int layers, char *smem, int c0, int dc, double *C, Input input)
{
	constexpr int NS = Fld<Q>::NS, W = EmsWide<Q>::W, NT = EmsWide<Q>::NT;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int nm = r.nm;

	double *U = (double *)smem;            // [maxdc][Q]  check-domain input vectors: U[j][h_j a] = v2c_j[a], U[j][0] = 0
	double *P = U + g.maxdc * Q;           // [layers][Q] DP state over the edges left of the current output edge
	double *A = P + layers * Q;            // [layers][Q] ping
	double *B = A + layers * Q;            // [layers][Q] pong
	double *Sv = B + layers * Q;           // [Q]         configuration-set maxima of the current output edge
	double *lv = Sv + Q;                   // [maxdc][nm] values of the nm most reliable entries (rank 0 first)
	int *lt = (int *)(lv + g.maxdc * nm);  // [maxdc][nm] their check-domain symbols

	// ---- stage: wave w takes edges w, w + W, .. (ems_check_node's staging, per edge) -------------------------------------------
	for (int j = wave; j < dc; j += W) {
		const auto vj = input(j);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + j], g.poly, lane);
		double v[NS];
		int t[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q && a > 0) ? vj(a) : 0.0;
			t[i] = mh.at_slot(i);
			if (a < Q) U[j * Q + t[i]] = v[i];
		}
		uint64_t member[NS];
		double top_v;
		int top_a;
		select_top<NS>(v, lane, Q, nm, member, top_v, top_a);
		// compact the members into the list, rank 0 swapped to the front
		int base = 0, p0 = 0;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			if (i == (top_a >> 6)) p0 = base + __popcll(member[i] & ((1ull << (top_a & 63)) - 1ull));
			base += __popcll(member[i]);
		}
		base = 0;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if ((member[i] >> lane) & 1ull) {
				int pos = base + prefix_count(member[i]);
				if (a == top_a) pos = 0;
				else if (pos == 0) pos = p0;
				lv[j * nm + pos] = v[i];
				lt[j * nm + pos] = t[i];
			}
			base += __popcll(member[i]);
		}
	}
	// the empty prefix: check sum 0 with no deviation at value 0.0, nothing else reachable
	for (int idx = tid; idx < layers * Q; idx += NT) P[idx] = (idx == 0) ? 0.0 : NBL_NEG_INF;
	__syncthreads();

	const int sym = tid;
	const bool own = Q >= 64 || sym < Q;
	int zsum = 0;
	for (int j = 0; j < dc; j++) zsum ^= lt[j * nm];

	// ---- one output edge at a time ---------------------------------------------------------------------------------------------
	for (int x = 0; x < dc; x++) {
		const int zall = zsum ^ lt[x * nm]; // the rank-0 symbols of the other edges
		double S = -NBL_DBL_MAX;

		// conf(q,1): at most one edge deviates, to ANY symbol.  For the deviating edge jd the candidate is the sum over the other edges
		// in index order; `pre` is its part left of jd, the same for every symbol
		double pre = 0.0;
		for (int jd = 0; jd < dc; jd++) {
			if (jd == x) continue;
			if (own) {
				double acc = pre + U[jd * Q + (sym ^ zall ^ lt[jd * nm])];
				int l = jd + 1;
				if (jd < x) {
					for (; l < x; l++) acc = acc + lv[l * nm];
					l = x + 1;
				}
				for (; l < dc; l++) acc = acc + lv[l * nm];
				S = dmax(S, acc);
			}
			pre = pre + lv[jd * nm];
		}

		// conf(nm,nc): at most nc edges deviate, each inside its nm best; conf(nm,0) is the all-rank-0 configuration alone, which
		// conf(q,1) already holds
		if (r.nc >= 1) {
			// Three buffers: the prefix P (read only, here) and ping / pong.  `cur` is the state the next step reads, `wr` the one of ping /
			// pong it writes, `oth` the other one.  A step reads cur and writes wr; after the barrier wr is current, and what was current
			// -- P, or oth since the swap -- has no reader left, so the swap makes it the next step's target
			const double *cur = P;
			double *wr = A, *oth = B;
			for (int l = x + 1; l < dc; l++) {
				ems_wide_step<Q>(cur, wr, lv + l * nm, lt + l * nm, nm, layers, sym, own);
				__syncthreads();
				cur = wr;
				double *t = wr;
				wr = oth;
				oth = t;
			}
			for (int d = 0; d < layers; d++)
				if (own) S = dmax(S, cur[d * Q + sym]); // (each thread reads what it wrote itself)
			// Advance the prefix by edge x.  Target: wr, which is not cur, and whose last readers (the step before the last) passed a
			// barrier.  The new prefix is read first after the barrier behind the Sv store below; the old one becomes ping, and is
			// written first by the next output edge's first step, after that same barrier
			if (x + 1 < dc) {
				ems_wide_step<Q>(P, wr, lv + x * nm, lt + x * nm, nm, layers, sym, own);
				double *old_prefix = P;
				P = wr;
				A = old_prefix;
				B = oth;
			}
		}

		// ---- output: c2v[a] = shape(S[h_x a] - S[0]) ----------------------------------------------------------------------------
		if (own) Sv[sym] = S;
		__syncthreads();
		{
			GfMul<Q> mh;
			mh.init(g.c_h[c0 + x], g.poly, lane);
			const double s0 = Sv[0];
			double *Cx = C + (size_t)x * Q;
			if (own) Cx[sym] = (sym == 0) ? 0.0 : shape_llr(Sv[mh.at_slot(wave)] - s0, r.factor, r.offset);
		}
		__syncthreads(); // Sv is rewritten by the next output edge
	}
}
