// nbldpc_amd/csrc/nbl_cn_bp_wide_core.h -- the exact log-domain QSPA check-node programme (nbl_cn_bp_core.h) in a layout whose LDS grows
// with (maxdc + 5) q instead of (3 maxdc + 5) q and that spreads one check over max(1, q / 64) waves: what runs checks of degree 9 ..
// NBL_BP_MAX_CHECK_DEGREE (nbl_create_bp_wide; kernels in nbl_cn_bp_wide.hip, flooding and layered).
//
// The programme is bp_check_node operation for operation: inputs into the check domain, F_1 = p_0, F_{k+1} = conv(F_k, p_k),
// R_{dc-2} = p_{dc-1}, R_{k-1} = conv(R_k, p_k), output 0 = R_0, output dc-1 = F_{dc-1}, otherwise conv(F_d, R_d), read at h_d a.  conv
// is lse_conv: the same extremes (a maximum does not depend on the order it is taken in), the same wave-uniform -- here
// workgroup-uniform -- narrow / wide decision at 650 nats, one exponential per input entry, one FMA or one ldexp pair per term IN
// ASCENDING x, one log per output, normalisation by output 0, first operand and second operand as there.  Every output's sum runs over x
// in the same order whatever thread owns it, so on a check both layouts can run the two give the same bits
// (tests/test_gpu_bp_wide.py holds them to that).  What differs is who holds what:
//
//   one check per WORKGROUP of W = max(1, Q / 64) waves.  Wave w stages edges w, w + W, .. through the per-wave input formers of
//   nbl_cn_bp_inputs.h; a WORKGROUP barrier follows.  From there on thread s owns symbol s alone (Q < 64: the lanes below Q).
//
//   a convolution takes its two operands and returns its result in the owner's registers: entry s of either operand is needed by thread s
//   alone (its exponential, its share of the extremes); what the other threads need are the exponentials, which go through the two [Q]
//   blocks PA / PB as in lse_conv.
//
//   F_d (d >= 1) lives in the check's own c2v region C[d] until that region's final store: thread s writes slot s, reads back slot s and
//   later stores the final c2v entry s over it -- program order of one thread at one address is all the ordering this needs.  The
//   outputs are produced from the last edge down while the running R advances in a register per thread, so neither F nor R needs a
//   [maxdc][Q] block.
//
// LDS: [maxdc][Q] check-domain inputs, one [Q] output vector, the two [Q] XP blocks, 32 doubles for the extremes of the waves and the
// normalising entry: (maxdc + 5) q 8 + 256 bytes, 76,032 B at q = 256 and degree 32 -- below the 160 KB of a workgroup for every shape
// the ABI accepts, so no shape is refused for LDS; above 64 KB the launcher opts in.
//
// Aliasing (the layered schedule).  input() of EVERY wave reads C (the check's own c2v) and the c2v of the neighbours.  The first write
// into C is the F_1 store of the forward pass; it comes after the workgroup barrier that follows the staging loop, and every thread
// reaches that barrier only after the loads of its own input() calls have returned (their values went into LDS before it).  So no
// wave's input() can see an F_d of another wave.  The checks of a layer share no variable, so no other workgroup reads or writes C.
//
// Every barrier is in workgroup-uniform control flow: dc, the loop counters and the narrow / wide decision (formed from the reduced
// extremes, which every thread holds identically) are uniform; the caller's early returns are per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_cn_bp_core.h" // XP

template <int Q> struct BpWide {
	static constexpr int W = Q >= 64 ? Q / 64 : 1; // waves of a check's workgroup
	static constexpr int NT = 64 * W;
};

#define NBL_BP_WIDE_RED_DOUBLES 32 // 4 extremes of at most 4 waves, the normalising entry at [16]

// lse_conv on operands held by their owners: returns out[s] = LSE_x(L1[x] + L2[s^x]) - LSE_x(L1[x] + L2[x]) (0 for s = 0), where
// thread s passes l1 = L1[s], l2 = L2[s].  PA, PB: [Q] XP in LDS; red: NBL_BP_WIDE_RED_DOUBLES doubles in LDS.  Called by the whole
// workgroup.  On return PA / PB / red may be rewritten at once (the last barrier follows their last read).
template <int Q>
__device__ __forceinline__ double lse_conv_wide(double l1, double l2, XP *PA, XP *PB, double *red, int s, bool own)
{
	constexpr int W = BpWide<Q>::W;
	const int sb = own ? s : 0; // (a thread without a symbol computes on symbol 0's addresses and stores nothing)
	double m1 = wave_fmax(own ? l1 : NBL_NEG_INF), m2 = wave_fmax(own ? l2 : NBL_NEG_INF);
	double n1 = wave_fmin(own ? l1 : __builtin_huge_val()), n2 = wave_fmin(own ? l2 : __builtin_huge_val());
	if (W > 1) {
		if ((s & 63) == 0) {
			double *mine = red + 4 * (s >> 6);
			mine[0] = m1; mine[1] = m2; mine[2] = n1; mine[3] = n2;
		}
		__syncthreads();
		// every thread folds the same W words in the same order: the decision below is the same in all of them whatever the inputs hold
		m1 = red[0]; m2 = red[1]; n1 = red[2]; n2 = red[3];
#pragma unroll
		for (int w = 1; w < W; w++) {
			m1 = dmax(m1, red[4 * w + 0]); m2 = dmax(m2, red[4 * w + 1]);
			n1 = dmin(n1, red[4 * w + 2]); n2 = dmin(n2, red[4 * w + 3]);
		}
	}
	const bool narrow = fmin(m1 - n1, m2 - n2) < 650.0; // workgroup-uniform
	double lse;
	if (narrow) {
		double *A = (double *)PA, *B = (double *)PB;
		if (own) { A[s] = exp(l1 - m1); B[s] = exp(l2 - m2); }
		__syncthreads();
		double acc = 0.0;
#pragma unroll 4
		for (int x = 0; x < Q; x++) acc = __fma_rn(A[x], B[sb ^ x], acc);
		lse = (log(acc) + m1) + m2;
	} else {
		const double LOG2E = 1.4426950408889634, LN2 = 0.6931471805599453;
		if (own) {
			const double y1 = (l1 - m1) * LOG2E, y2 = (l2 - m2) * LOG2E;
			const double f1 = floor(y1), f2 = floor(y2);
			XP a, b;
			a.m = exp2(y1 - f1); a.e = (int)dmax(f1, -1.0e9); a.pad = 0;
			b.m = exp2(y2 - f2); b.e = (int)dmax(f2, -1.0e9); b.pad = 0;
			PA[s] = a;
			PB[s] = b;
		}
		__syncthreads();
		double acc = 0.0;
		int ex = -2000000000;
#pragma unroll 2
		for (int x = 0; x < Q; x++) {
			const XP a = PA[x];
			const XP b = PB[sb ^ x];
			const int e = a.e + b.e;
			const int top = e > ex ? e : ex;
			// both rescalings are exact (power of two); differences beyond the double range give 0
			const int d0 = ex - top, d1 = e - top;
			acc = ldexp(acc, d0 < -2000 ? -2000 : d0) + ldexp(a.m * b.m, d1 < -2000 ? -2000 : d1);
			ex = top;
		}
		lse = ((log(acc) + (double)ex * LN2) + m1) + m2;
	}
	if (s == 0) red[16] = lse; // b = 0
	__syncthreads();
	const double norm = red[16];
	return (s == 0) ? 0.0 : lse - norm;
}

// One check of `dc` edges starting at check-major edge c0, by the calling workgroup of BpWide<Q>::NT threads; `smem` is its dynamic LDS
// (nbl_bp_wide_lds_bytes).  input(d, v) and C as for bp_check_node; input is called by ONE wave per edge (wave d % W), in that wave's edge
// order, and only before the first workgroup barrier.
template <int Q, class Input>
__device__ __forceinline__ void bp_wide_check_node(const NblGraphDev &g, char *smem, int c0, int dc, double *C, Input input)
{
	constexpr int NS = Fld<Q>::NS, W = BpWide<Q>::W;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int mdc = g.maxdc;

	double *Pp = (double *)smem;   // [mdc][Q] inputs in the check domain
	double *T = Pp + mdc * Q;      // [Q] the output vector before its permutation
	XP *PA = (XP *)(T + Q);        // [Q] e^(L1 - max), plain double or mantissa/exponent
	XP *PB = PA + Q;               // [Q] e^(L2 - max)
	double *red = (double *)(PB + Q);

	for (int d = wave; d < dc; d += W) {
		double v[NS];
		input(d, v);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) Pp[d * Q + mh.at_slot(i)] = (a == 0) ? 0.0 : v[i];
		}
	}
	__syncthreads(); // every input() of every wave is complete: C is free from here on

	const int s = tid;
	const bool own = Q >= 64 || s < Q;
	const int sb = own ? s : 0;
	// forward partials: F_1 = p_0, F_{k+1} = conv(F_k, p_k); F_k parked in C[k][s]
	double f = Pp[sb];
#pragma unroll 1
	for (int k = 1; k + 1 <= dc - 1; k++) {
		if (own) C[(size_t)k * Q + s] = f;
		f = lse_conv_wide<Q>(f, Pp[k * Q + sb], PA, PB, red, s, own);
	}
	// from the last edge down: r = R_d, R_{dc-2} = p_{dc-1}, R_{d-1} = conv(R_d, p_d)
	double r = Pp[(dc - 1) * Q + sb];
#pragma unroll 1
	for (int d = dc - 1; d >= 0; d--) {
		double *Cd = C + (size_t)d * Q;
		double val;
		if (d == dc - 1) val = f;      // A2 = 0: F_{dc-1}
		else if (d == 0) val = r;      // A1 = 0: R_0
		else {
			const double fd = own ? Cd[s] : 0.0; // F_d, this thread's own store
			val = lse_conv_wide<Q>(fd, r, PA, PB, red, s, own);
		}
		if (own) T[s] = val;
		__syncthreads();
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
		if (own) Cd[s] = (s == 0) ? 0.0 : T[mh.at_slot(wave)];
		__syncthreads(); // T is rewritten by the next output
		if (d >= 1 && d <= dc - 2) r = lse_conv_wide<Q>(r, Pp[d * Q + sb], PA, PB, red, s, own);
	}
}
