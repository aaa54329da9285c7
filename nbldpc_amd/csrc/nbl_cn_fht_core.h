// nbldpc_amd/csrc/nbl_cn_fht_core.h -- the FHT sum-product check-node programme of include/nbldpc.h (nbl_create_fht), shared by the
// flooding kernel (nbl_cn_fht.hip) and the layered kernel (nbl_cn_fht_layered.hip): one wave per check, the same device code in both.
//
// Over GF(2^p) the box-plus of the sum-product rule is an XOR convolution of probability vectors (nbl_cn_bp_core.h derives it), and
// the Walsh-Hadamard transform turns an XOR convolution into a pointwise product.  A check of degree dc therefore costs dc forward
// transforms, 3 dc - 4 pointwise products and dc inverse transforms of q log2 q butterflies each, instead of 3 (dc - 2) sums of q^2
// terms.  The transform subtracts: what comes out far below a vector's largest entry is rounding noise, so every output is floored at
// 2^-NBL_FHT_FLOOR_LOG2 of its vector's maximum.  That makes this a method of its own, defined operation by operation in the header
// (steps 1-7 below are the header's), not another evaluation of nbl_cn_bp_core.h's statement.
//
// Layout: a lane holds slots lane + 64 i, i < NS, of every vector (lanes >= Q hold zeros when Q < 64: they take part in no butterfly
// with a lane below Q, because only strides below Q run).  A butterfly of stride 64 or 128 pairs two registers of one lane; a stride
// below 64 pairs this lane with lane ^ stride: quad permutes on the DPP network (1, 2), ds_swizzle in bit mode (4, 8, 16: no address
// register, no LDS traffic), ds_bpermute across the two halves (32).  The lane that owns the upper slot computes partner - own, the
// other own + partner: the same two roundings as the header's (x[i] + x[i+s], x[i] - x[i+s]).
//
// Storage: the transformed inputs U_k stay in registers (DCM x NS doubles per lane; the loops over edges are unrolled over DCM with
// wave-uniform guards, so no array is indexed dynamically; degrees above DCM = 8 run the layout of nbl_cn_fht_wide_core.h instead).  LDS
// holds ONE [maxdc][Q] block of doubles -- at most 16 KB at degree 8 -- which serves
// three times: the permutation by h_d on the way in, the forward products Fwd_k while the outputs are formed from the last edge down,
// and the permutation back on the way out (region d is read as Fwd_d by the lane that then overwrites the same slots with c_d).
// DESIGN.md section 5l has the register report behind that split.
//
// Contract (that of bp_check_node): the check is (c0, dc); input(d, v) is called once per edge, in edge order, by the whole wave, and
// ONLY in step 1, before the first barrier; C ([dc][Q]) is written in the last step alone, so every read input() makes is complete
// before the first output is stored and C may alias what input() reads.  `smem` is the wave's dynamic LDS (nbl_fht_lds_bytes).
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "../../include/nbldpc.h"

inline size_t nbl_fht_lds_bytes(size_t q, size_t mdc) { return mdc * q * 8; }

// the value lane ^ S holds, S < 64
template <int S> __device__ __forceinline__ double fht_partner(double x)
{
	if constexpr (S == 1) return dpp_f64<0xB1, 0xF>(x);      // quad_perm [1,0,3,2]
	else if constexpr (S == 2) return dpp_f64<0x4E, 0xF>(x); // quad_perm [2,3,0,1]
	else if constexpr (S == 32) return __shfl_xor(x, 32, 64);
	else { // bit mode: lane' = ((lane & 0x1f) | 0) ^ S inside each half of the wave
		constexpr int pat = 0x1f | (S << 10);
		return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(x), pat), __builtin_amdgcn_ds_swizzle(__double2loint(x), pat));
	}
}

template <int Q, int S> __device__ __forceinline__ void fht_lane_stage(double (&x)[Fld<Q>::NS], int lane)
{
	if constexpr (S < Q && S < 64) {
		const bool upper = (lane & S) != 0;
#pragma unroll
		for (int i = 0; i < Fld<Q>::NS; i++) {
			const double o = fht_partner<S>(x[i]);
			x[i] = upper ? o - x[i] : x[i] + o;
		}
	}
}

// x <- WHT(x), unnormalised: strides 1, 2, 4, .., Q/2 in that order
template <int Q> __device__ __forceinline__ void fht(double (&x)[Fld<Q>::NS], int lane)
{
	fht_lane_stage<Q, 1>(x, lane);
	fht_lane_stage<Q, 2>(x, lane);
	fht_lane_stage<Q, 4>(x, lane);
	fht_lane_stage<Q, 8>(x, lane);
	fht_lane_stage<Q, 16>(x, lane);
	fht_lane_stage<Q, 32>(x, lane);
	if constexpr (Q >= 128) { // stride 64: slots (0,1) and (2,3)
#pragma unroll
		for (int i = 0; i + 1 < Fld<Q>::NS; i += 2) {
			const double a = x[i], b = x[i + 1];
			x[i] = a + b;
			x[i + 1] = a - b;
		}
	}
	if constexpr (Q >= 256) { // stride 128: slots (0,2) and (1,3)
#pragma unroll
		for (int i = 0; i < 2; i++) {
			const double a = x[i], b = x[i + 2];
			x[i] = a + b;
			x[i + 2] = a - b;
		}
	}
}

// DCM: the largest degree the unrolled edge loops cover (the launcher takes 4 when the code has no larger check: half the registers)
template <int Q, class Input, int DCM = NBL_MAXDC>
__device__ __forceinline__ void fht_check_node(const NblGraphDev &g, char *smem, int c0, int dc, double *C, Input input)
{
	constexpr int NS = Fld<Q>::NS;
	const int lane = lane_id();
	double *S = (double *)smem; // [maxdc][Q]

	// 1. the check domain: p_d[h_d a] = in_d[a]
	for (int d = 0; d < dc; d++) {
		double v[NS];
		input(d, v);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) S[d * Q + mh.at_slot(i)] = (a == 0) ? 0.0 : v[i];
		}
	}
	__syncthreads();
	// 2., 3. u_d = exp(p_d - max p_d), U_d = WHT(u_d)
	double U[DCM][NS];
#pragma unroll
	for (int d = 0; d < DCM; d++) {
		if (d < dc) {
			double m = NBL_NEG_INF;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				U[d][i] = (y < Q) ? S[d * Q + y] : NBL_NEG_INF;
				m = dmax(m, U[d][i]);
			}
			m = wave_fmax(m);
#pragma unroll
			for (int i = 0; i < NS; i++) U[d][i] = (lane + 64 * i < Q) ? exp(U[d][i] - m) : 0.0;
			fht<Q>(U[d], lane);
		}
	}
	// 4. forward products into LDS (own slots: region k is read and written by the same lanes at the same addresses from here on)
	{
		double F[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) F[i] = U[0][i];
#pragma unroll
		for (int k = 1; k < DCM; k++) {
			if (k < dc) {
#pragma unroll
				for (int i = 0; i < NS; i++) {
					int y = lane + 64 * i;
					if (y < Q) S[k * Q + y] = F[i];        // Fwd_k
					F[i] = F[i] * U[k][i];                 // Fwd_{k+1}
				}
			}
		}
	}
	// 4.-7. from the last edge down, with the running backward product
	double Bw[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) Bw[i] = 0.0;
#pragma unroll
	for (int d = DCM - 1; d >= 0; d--) {
		if (d < dc) {
			double v[NS];
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				const double f = (y < Q && d > 0) ? S[d * Q + y] : 0.0;
				v[i] = (d == dc - 1) ? f : (d == 0) ? Bw[i] : f * Bw[i]; // V_d
			}
			// Bwd_{d-1}: Bwd_{dc-2} = U_{dc-1}, Bwd_{k-1} = Bwd_k U_k
#pragma unroll
			for (int i = 0; i < NS; i++) Bw[i] = (d == dc - 1) ? U[d][i] : Bw[i] * U[d][i];
			fht<Q>(v, lane); // 5.
			double t = NBL_NEG_INF;
#pragma unroll
			for (int i = 0; i < NS; i++)
				if (lane + 64 * i < Q) t = dmax(t, v[i]);
			t = wave_fmax(t);
			const double fl = t * (1.0 / (double)(1ull << NBL_FHT_FLOOR_LOG2)); // 6. (a power of two: exact)
#pragma unroll
			for (int i = 0; i < NS; i++) v[i] = log(dmax(v[i], fl));
			const double l0 = read_lane_f64(v[0], 0); // 7.
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				if (y < Q) S[d * Q + y] = v[i] - l0;
			}
			__syncthreads();
			GfMul<Q> mh;
			mh.init(g.c_h[c0 + d], g.poly, lane);
			double *Cd = C + (size_t)d * Q;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				if (a < Q) Cd[a] = (a == 0) ? 0.0 : S[d * Q + mh.at_slot(i)];
			}
		}
	}
}
