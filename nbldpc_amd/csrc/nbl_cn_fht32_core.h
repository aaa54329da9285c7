// nbldpc_amd/csrc/nbl_cn_fht32_core.h -- the single-precision FHT sum-product check-node programme of include/nbldpc.h
// (nbl_create_fht32), shared by the flooding and the layered kernel of nbl_cn_fht32.hip: one wave per check, the same device code in both.
//
// It is nbl_cn_fht_core.h (which derives the method) in IEEE binary32: the same steps 1-7 in the same order, the floor at
// 2^-NBL_FHT32_FLOOR_LOG2 of a vector's maximum, expf / logf of the device library (within 2 ulp, what the header allows).  The file is
// compiled with -ffp-contract=off like the rest of the library: every product and every sum is rounded on its own.
//
// Layout: that of the FP64 programme -- a lane holds slots lane + 64 i, i < NS, of every vector (lanes >= Q hold zeros when Q < 64).  A
// value is one register, so a butterfly of stride below 64 is ONE cross-lane exchange where the FP64 programme needs two: a DPP quad
// permute (1, 2), a ds_swizzle in bit mode (4, 8, 16), a ds_bpermute across the two halves (32).  Strides 64 and 128 pair two registers
// of one lane.  The lane that owns the upper slot computes partner - own, the other own + partner.
//
// Storage: the transformed inputs U_k stay in registers (DCM x NS floats per lane: 32 VGPRs at Q = 256, DCM = 8); LDS holds ONE
// [maxdc][Q] block of floats -- at most 8 KB -- serving the same three purposes as in the FP64 programme (permutation in, forward
// products, permutation out).  Degrees above DCM = 8 are not run: |U[y]| <= Q, so the product of 7 transformed vectors stays below
// 2^56 and its transform below 2^64, inside binary32's range; at degree 32 it would leave it (nbl_create_fht32 refuses such a code).
//
// Contract: that of fht_check_node.  `smem` is the wave's dynamic LDS (nbl_fht32_lds_bytes).
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "../../include/nbldpc.h"

inline size_t nbl_fht32_lds_bytes(size_t q, size_t mdc) { return mdc * q * 4; }

#define NBL_NEG_INF_F (-__builtin_huge_valf())

// (the wave helpers on floats -- fmax32, dpp_f32, wave_fmax32, wave_decide32 -- are in nbl_device.h, beside the FP64 ones)

// the value lane ^ S holds, S < 64: one exchange
template <int S> __device__ __forceinline__ float fht32_partner(float x)
{
	if constexpr (S == 1) return dpp_f32<0xB1, 0xF>(x);      // quad_perm [1,0,3,2]
	else if constexpr (S == 2) return dpp_f32<0x4E, 0xF>(x); // quad_perm [2,3,0,1]
	else if constexpr (S == 32) return __shfl_xor(x, 32, 64);
	else { // bit mode: lane' = (lane & 0x1f) ^ S inside each half of the wave
		constexpr int pat = 0x1f | (S << 10);
		return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), pat));
	}
}

template <int Q, int S> __device__ __forceinline__ void fht32_lane_stage(float (&x)[Fld<Q>::NS], int lane)
{
	if constexpr (S < Q && S < 64) {
		const bool upper = (lane & S) != 0;
#pragma unroll
		for (int i = 0; i < Fld<Q>::NS; i++) {
			const float o = fht32_partner<S>(x[i]);
			x[i] = upper ? o - x[i] : x[i] + o;
		}
	}
}

// x <- WHT(x), unnormalised: strides 1, 2, 4, .., Q/2 in that order
template <int Q> __device__ __forceinline__ void fht32(float (&x)[Fld<Q>::NS], int lane)
{
	fht32_lane_stage<Q, 1>(x, lane);
	fht32_lane_stage<Q, 2>(x, lane);
	fht32_lane_stage<Q, 4>(x, lane);
	fht32_lane_stage<Q, 8>(x, lane);
	fht32_lane_stage<Q, 16>(x, lane);
	fht32_lane_stage<Q, 32>(x, lane);
	if constexpr (Q >= 128) { // stride 64: slots (0,1) and (2,3)
#pragma unroll
		for (int i = 0; i + 1 < Fld<Q>::NS; i += 2) {
			const float a = x[i], b = x[i + 1];
			x[i] = a + b;
			x[i + 1] = a - b;
		}
	}
	if constexpr (Q >= 256) { // stride 128: slots (0,2) and (1,3)
#pragma unroll
		for (int i = 0; i < 2; i++) {
			const float a = x[i], b = x[i + 2];
			x[i] = a + b;
			x[i + 2] = a - b;
		}
	}
}

// DCM: the largest degree the unrolled edge loops cover (the launcher takes 4 when the code has no larger check: half the registers)
template <int Q, class Input, int DCM = NBL_MAXDC>
__device__ __forceinline__ void fht32_check_node(const NblGraphDev &g, char *smem, int c0, int dc, float *C, Input input)
{
	constexpr int NS = Fld<Q>::NS;
	const int lane = lane_id();
	float *S = (float *)smem; // [maxdc][Q]

	// 1. the check domain: p_d[h_d a] = in_d[a]
	for (int d = 0; d < dc; d++) {
		float v[NS];
		input(d, v);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) S[d * Q + mh.at_slot(i)] = (a == 0) ? 0.0f : v[i];
		}
	}
	__syncthreads();
	// 2., 3. u_d = exp(p_d - max p_d), U_d = WHT(u_d)
	float U[DCM][NS];
#pragma unroll
	for (int d = 0; d < DCM; d++) {
		if (d < dc) {
			float m = NBL_NEG_INF_F;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				U[d][i] = (y < Q) ? S[d * Q + y] : NBL_NEG_INF_F;
				m = fmax32(m, U[d][i]);
			}
			m = wave_fmax32(m);
#pragma unroll
			for (int i = 0; i < NS; i++) U[d][i] = (lane + 64 * i < Q) ? expf(U[d][i] - m) : 0.0f;
			fht32<Q>(U[d], lane);
		}
	}
	// 4. forward products into LDS (own slots: region k is read and written by the same lanes at the same addresses from here on)
	{
		float F[NS];
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
	float Bw[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) Bw[i] = 0.0f;
#pragma unroll
	for (int d = DCM - 1; d >= 0; d--) {
		if (d < dc) {
			float v[NS];
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				const float f = (y < Q && d > 0) ? S[d * Q + y] : 0.0f;
				v[i] = (d == dc - 1) ? f : (d == 0) ? Bw[i] : f * Bw[i]; // V_d
			}
			// Bwd_{d-1}: Bwd_{dc-2} = U_{dc-1}, Bwd_{k-1} = Bwd_k U_k
#pragma unroll
			for (int i = 0; i < NS; i++) Bw[i] = (d == dc - 1) ? U[d][i] : Bw[i] * U[d][i];
			fht32<Q>(v, lane); // 5.
			float t = NBL_NEG_INF_F;
#pragma unroll
			for (int i = 0; i < NS; i++)
				if (lane + 64 * i < Q) t = fmax32(t, v[i]);
			t = wave_fmax32(t);
			const float fl = t * (1.0f / (float)(1u << NBL_FHT32_FLOOR_LOG2)); // 6. (a power of two: exact)
#pragma unroll
			for (int i = 0; i < NS; i++) v[i] = logf(fmax32(v[i], fl));
			const float l0 = read_lane_f32(v[0], 0); // 7.
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				if (y < Q) S[d * Q + y] = v[i] - l0;
			}
			__syncthreads();
			GfMul<Q> mh;
			mh.init(g.c_h[c0 + d], g.poly, lane);
			float *Cd = C + (size_t)d * Q;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				if (a < Q) Cd[a] = (a == 0) ? 0.0f : S[d * Q + mh.at_slot(i)];
			}
		}
	}
}
