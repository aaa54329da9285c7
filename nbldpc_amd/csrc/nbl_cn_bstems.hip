// nbldpc_amd/csrc/nbl_cn_bstems.hip -- basic-set T-EMS check node (decode method 7; DESIGN.md sections 1 and 3).
//
// One wave per (codeword, check); lane l owns symbols l + 64 i.  Steps:
//   a. beta_d, syndrome, delta-domain dU[d][eta] (as T-EMS), and per symbol the two smallest columns of a stable ascending
//      order of dU[.][s] (ties: the lower column first).  LLV[s] = dU[Min0[s]][s] >= 0, LLV[0] = 0.
//   b. the basic set, `nm` elements (symbol, column Min0, cost LLV), symbols ordered by the key (LLV, s):
//        nm >  p: the nm smallest non-zero keys;
//        nm <= p: the first nm vectors of the greedy GF(2) basis along that order (each symbol not in the span of those
//                 already taken).  Walking the order and taking every symbol outside the span = repeatedly taking the
//                 smallest key outside the span, so both cases are nm rounds of a masked wave argmin; the span test is at
//                 most p XORs against an echelon basis held in registers (uniform over the wave).
//   c. the configurations: subsets of the elements with pairwise different columns and at most nc members.  A subset's
//      cost is the left-to-right sum of its elements' LLV in element order, its check sum the XOR of their symbols.  The
//      reference's DFS (include before exclude, element 0 first) keeps, per check sum, the first configuration of minimal
//      cost: the one with the LARGEST inclusion mask read with element 0 as the most significant bit.  Here the subsets are
//      spread over the lanes (every mask below 2^nm, those with more than nc members or a repeated column skipped) and the
//      per-symbol minimum of (cost, DFS rank) is taken in LDS: a fetch_min of the cost, then a fetch_max of the rank among
//      the configurations that reach it.  Check sum 0 keeps dW = 0 and the all-zero Eta (no configuration costs less).
//   d. the T-EMS output stage: extrinsic minimum per edge, fill of unreached symbols from the two smallest columns, back to
//      the normal domain with the BS-TEMS factor / offset.
// The reference keeps the configuration cost as a running sum (+= on the way in, -= on the way out); its residue is not
// reproduced, and exact ties in LLV are ordered by symbol.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"

#define NBL_BS_MAXNM 16

template <int Q>
__global__ __launch_bounds__(64) void cn_bstems_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	constexpr int NS = Fld<Q>::NS;
	constexpr int P = Fld<Q>::P;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int lane = lane_id();
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const int c0 = k.c0, dc = k.dc;
	const int nm = r.nm, nc = r.nc, mdc = g.maxdc;

	double *dU = (double *)smem;                   // [mdc][Q]
	double *Lc = dU + mdc * Q;                     // [Q] extrinsic vector of one edge
	double *Wv = Lc + Q;                           // [Q] cheapest configuration per check sum
	double *elL = Wv + Q;                          // [NBL_BS_MAXNM] element costs
	unsigned *Wk = (unsigned *)(elL + NBL_BS_MAXNM); // [Q] DFS rank of the first cheapest configuration (0 = none)
	int *ord01 = (int *)(Wk + Q);                  // [Q] two smallest columns per symbol (lo byte, next byte)
	int *elq = ord01 + Q;                          // [NBL_BS_MAXNM] element symbols
	int *elc = elq + NBL_BS_MAXNM;                 // [NBL_BS_MAXNM] element columns
	int *beta = elc + NBL_BS_MAXNM;                // [mdc]

	const double *V = w.v2c + (size_t)b * g.E * Q;
	double *C = w.c2v + ((size_t)b * g.E + c0) * Q;

	// ---- a. beta, syndrome, dU (TEMS_Get_Beta / TEMS_Get_deltaU) -------------------------------------------------------
	int syn = 0;
	for (int d = 0; d < dc; d++) {
		const double *Vd = V + (size_t)g.c_epos[c0 + d] * Q;
		double v[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q && a > 0) ? Vd[a] : 0.0;
		}
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
		int bd = 0; // beta_d = h * argmax (0 if nothing positive)
		{
			int x = g.c_h[c0 + d];
			for (int k = 0; k < 8; k++) {
				if ((arg >> k) & 1) bd ^= x;
				x <<= 1;
				if (x & Q) x ^= g.poly;
			}
		}
		bd = uniform(bd);
		const double mx = uniform_f64(best);
		if (lane == 0) beta[d] = bd;
		syn ^= bd;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) dU[d * Q + (mh.at_slot(i) ^ bd)] = mx - v[i];
		}
	}
	__syncthreads();

	// per symbol: the two smallest columns (stable), LLV
	double llv[NS];
	int col0[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) {
		const int s = lane + 64 * i;
		llv[i] = 0.0;
		col0[i] = 0;
		if (s < Q) {
			int b0 = 0, b1 = -1;
			double u0 = dU[s], u1 = 0.0;
			for (int d = 1; d < dc; d++) {
				const double u = dU[d * Q + s];
				if (u < u0) { b1 = b0; u1 = u0; b0 = d; u0 = u; }
				else if (b1 < 0 || u < u1) { b1 = d; u1 = u; }
			}
			ord01[s] = b0 | (b1 << 8);
			llv[i] = u0;
			col0[i] = b0;
		}
	}

	// ---- b. the basic set: nm rounds of a masked argmin of (LLV, s) -----------------------------------------------------
	const bool greedy = nm <= P;
	int ech[P];      // echelon basis of the span so far: ech[k] has leading bit k (0 = none); uniform
#pragma unroll
	for (int k = 0; k < P; k++) ech[k] = 0;
	unsigned taken = 0; // bit i: symbol lane + 64 i is an element (nm > p)
	for (int k = 0; k < nm; k++) {
		double best = __builtin_huge_val();
		int bs = Q, bcol = 0;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			const int s = lane + 64 * i;
			bool ok = s > 0 && s < Q;
			if (greedy) {
				int t = s;
#pragma unroll
				for (int bit = P - 1; bit >= 0; bit--)
					if ((t >> bit) & 1) t ^= ech[bit];
				ok = ok && t != 0;
			} else {
				ok = ok && !((taken >> i) & 1);
			}
			// ascending s per lane: strict '<' keeps the smaller symbol on equal LLV
			if (ok && llv[i] < best) { best = llv[i]; bs = s; bcol = col0[i]; }
		}
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			const double ob = __shfl_xor(best, off, 64);
			const int os = __shfl_xor(bs, off, 64), oc = __shfl_xor(bcol, off, 64);
			if (ob < best || (ob == best && os < bs)) { best = ob; bs = os; bcol = oc; }
		}
		bs = uniform(bs) & (Q - 1); // (a symbol in every case: with non-finite inputs nothing may compare below +inf)
		if (lane == 0) { elq[k] = bs; elc[k] = uniform(bcol); elL[k] = uniform_f64(best); }
		if (greedy) {
			int t = bs;
#pragma unroll
			for (int bit = P - 1; bit >= 0; bit--)
				if ((t >> bit) & 1) t ^= ech[bit];
			// t != 0 (bs is outside the span): it joins the basis at its leading bit
#pragma unroll
			for (int bit = P - 1; bit >= 0; bit--)
				if (t != 0 && (t >> bit) == 1) ech[bit] = t;
		} else {
#pragma unroll
			for (int i = 0; i < NS; i++)
				if (lane + 64 * i == bs) taken |= 1u << i;
		}
	}
	for (int s = lane; s < Q; s += 64) { Wv[s] = NBL_DBL_MAX; Wk[s] = 0; }
	__syncthreads();

	// ---- c. configurations: per check sum the cheapest, then the first in DFS order among the cheapest ------------------
	const unsigned nmask = 1u << nm;
	for (int pass = 0; pass < 2; pass++) {
		for (unsigned msk = lane; msk < nmask; msk += 64) {
			if (__builtin_popcount(msk) > nc) continue;
			unsigned cols = 0;
			int sym = 0;
			bool clash = false;
			double cost = 0.0;
			for (unsigned t = msk; t; t &= t - 1) { // elements in ascending order: the left-to-right sum
				const int e = __builtin_ctz(t);
				const unsigned cb = 1u << elc[e];
				clash = clash || (cols & cb);
				cols |= cb;
				sym ^= elq[e];
				cost = cost + elL[e];
			}
			if (clash || sym == 0) continue;
			if (pass == 0) {
				__hip_atomic_fetch_min(&Wv[sym], cost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			} else if (cost == Wv[sym]) {
				const unsigned rank = __builtin_bitreverse32(msk) >> (32 - nm); // element 0 = most significant bit
				__hip_atomic_fetch_max(&Wk[sym], rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			}
		}
		__syncthreads();
	}
	// dW, Eta (one byte per column) of the owned symbols
	double dW[NS];
	unsigned long long eta[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) {
		const int s = lane + 64 * i;
		dW[i] = NBL_DBL_MAX;
		eta[i] = 0;
		if (s == 0) dW[i] = 0.0;
		else if (s < Q && Wk[s] != 0) {
			dW[i] = Wv[s];
			const unsigned msk = __builtin_bitreverse32(Wk[s]) >> (32 - nm);
			for (unsigned t = msk; t; t &= t - 1) {
				const int e = __builtin_ctz(t);
				eta[i] |= (unsigned long long)elq[e] << (8 * elc[e]);
			}
		}
	}

	// ---- d. outputs (the T-EMS output stage) ------------------------------------------------------------------------------
	for (int d = 0; d < dc; d++) {
		__syncthreads();
		for (int s = lane; s < Q; s += 64) Lc[s] = NBL_DBL_MAX;
		__syncthreads();
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int s = lane + 64 * i;
			if (s < Q && dW[i] < NBL_DBL_MAX) {
				const int dev = (int)((eta[i] >> (8 * d)) & 255);
				const double cand = dW[i] - dU[d * Q + dev];
				__hip_atomic_fetch_min(&Lc[s ^ dev], cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			}
		}
		__syncthreads();
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int s = lane + 64 * i;
			if (s < Q && Lc[s] == NBL_DBL_MAX) { // never reached
				const int o0 = ord01[s] & 255, o1 = (ord01[s] >> 8) & 255;
				Lc[s] = (d == o0) ? dU[o1 * Q + s] : dU[o0 * Q + s];
			}
		}
		__syncthreads();
		// delta domain -> LLR, un-permute by h
		const int bsyn = syn ^ beta[d];
		const double L0 = -1.0 * Lc[bsyn];
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
		double *Cd = C + (size_t)d * Q;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) {
				const int e = mh.at_slot(i) ^ bsyn; // eta with h^-1 (eta ^ bsyn) = a
				Cd[a] = (a == 0) ? 0.0 : shape_llr(-1.0 * Lc[e] - L0, r.factor, r.offset);
			}
		}
	}
}

size_t nbl_bstems_lds_bytes(const NblGraphDev &g)
{
	const size_t q = g.q, mdc = g.maxdc;
	return (mdc * q + 2 * q + NBL_BS_MAXNM) * 8 + (2 * q + 2 * NBL_BS_MAXNM + mdc) * 4 + 64;
}

bool nbl_bstems_applicable(const NblGraphDev &g, int nm, int nc)
{
	return nm >= 1 && nm <= NBL_BS_MAXNM && nm < g.q && nc >= 0 && g.maxdc <= 8 && g.q >= 4 && g.q <= 256 &&
	       nbl_bstems_lds_bytes(g) <= NBL_LDS_OPT_IN;
}

hipError_t nbl_launch_cn_bstems(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	if (!nbl_bstems_applicable(g, r.nm, r.nc)) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_bstems_kernel<QQ>, (long long)r.B * g.M, 64, nbl_bstems_lds_bytes(g), st, g, w, r))
}
