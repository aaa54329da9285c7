// nbldpc_amd/csrc/nbl_cn_fht32.hip -- single-precision FHT sum-product check node (nbl_create_fht32): the programme of
// nbl_cn_fht32_core.h under the flooding schedule (one wave per (codeword, check), on the float v2c the variable-node pass of
// nbl_fht32.hip wrote) and under the damped layered schedule (the checks of one layer; each forms its inputs from Lf and the one float
// c2v buffer and damps them against the edge's float v2c, updated in place).  The launch shapes, and the argument for one c2v and one
// v2c buffer under the layered schedule, are those of nbl_cn_fht.hip / nbl_cn_fht_layered.hip.  q < 64 leaves lanes idle.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_fht32_core.h"

// flooding: entry lane + 64 i of edge d's v2c vector (BpV2cInput of nbl_cn_bp_inputs.h on floats)
template <int Q> struct Bp32V2cInput {
	const float *V;  // the codeword's v2c block
	const int *epos; // the check's row of c_epos
	int lane;
	__device__ __forceinline__ void operator()(int d, float (&v)[Fld<Q>::NS]) const
	{
		const float *Vd = V + (size_t)epos[d] * Q;
#pragma unroll
		for (int i = 0; i < Fld<Q>::NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Vd[a] : 0.0f;
		}
	}
};

// damped layered schedule (BpLayeredInput on floats): input of edge j, variable n: P = Lf[n], then + c2v of each of n's edges in n's
// order (the CURRENT values); raw = P - c2v of this edge; damped 0.5 / 0.5 against the stored v2c of this edge where the two decide
// differently; stored back as the edge's v2c.  Every operation in binary32.
template <int Q> struct Bp32LayeredInput {
	const float *L;  // the codeword's Lf block
	const float *Cb; // the codeword's c2v block
	float *Vb;       // the codeword's v2c block
	const int *nbr;  // NblLayerDev::nbr
	const int *epos; // NblGraphDev::c_epos
	int c0, lane;
	float damp_old, damp_new;
	__device__ __forceinline__ void operator()(int j, float (&v)[Fld<Q>::NS]) const
	{
		constexpr int NS = Fld<Q>::NS;
		const int *row = nbr + (size_t)(c0 + j) * NBL_LAYER_ROW;
		const int dv = row[1];
		const float *Ln = L + (size_t)row[0] * Q;
		const float *own = Cb + (size_t)(c0 + j) * Q;
		float *Vd = Vb + (size_t)epos[c0 + j] * Q;
		float ov[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Ln[a] : 0.0f;
			ov[i] = (a < Q) ? Vd[a] : 0.0f;
		}
		for (int d = 0; d < dv; d++) {
			const float *Cd = Cb + (size_t)row[4 + d] * Q;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				if (a < Q) v[i] = v[i] + Cd[a];
			}
		}
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) v[i] = v[i] - own[a];
		}
		const int before = wave_decide32<NS>(ov, lane, Q);
		const int after = wave_decide32<NS>(v, lane, Q);
		if (before != after) {
#pragma unroll
			for (int i = 0; i < NS; i++) v[i] = __fadd_rn(__fmul_rn(damp_old, ov[i]), __fmul_rn(damp_new, v[i]));
		}
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a == 0) v[i] = 0.0f;
			if (a < Q) Vd[a] = v[i];
		}
	}
};

template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht32_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const Bp32V2cInput<Q> in = {f.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	fht32_check_node<Q, Bp32V2cInput<Q>, DCM>(g, smem, c0, dc, f.c2v + ((size_t)b * g.E + c0) * Q, in);
}

// the checks of one layer: one wave per (codeword, check); grid = count * (codeword slots)
template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht32_layered_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / count), m = ly.chk[offset + blockIdx.x % count];
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	float *Cb = f.c2v + (size_t)b * g.E * Q;
	const Bp32LayeredInput<Q> input = {f.Lf + (size_t)b * g.N * Q, Cb, f.v2c + (size_t)b * g.E * Q, ly.nbr, g.c_epos, c0, lane_id(), (float)r.damp_old, (float)r.damp_new};
	fht32_check_node<Q, Bp32LayeredInput<Q>, DCM>(g, smem, c0, dc, Cb + (size_t)c0 * Q, input);
}

#define NBL_FHT32_Q(q, ...)                                     \
	switch (q) {                                                \
	case 4: { constexpr int QQ = 4; __VA_ARGS__; } break;       \
	case 8: { constexpr int QQ = 8; __VA_ARGS__; } break;       \
	case 16: { constexpr int QQ = 16; __VA_ARGS__; } break;     \
	case 32: { constexpr int QQ = 32; __VA_ARGS__; } break;     \
	case 64: { constexpr int QQ = 64; __VA_ARGS__; } break;     \
	case 128: { constexpr int QQ = 128; __VA_ARGS__; } break;   \
	case 256: { constexpr int QQ = 256; __VA_ARGS__; } break;   \
	default: return hipErrorInvalidValue;                       \
	}

hipError_t nbl_launch_cn_fht32(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, hipStream_t st)
{
	// maxdc q 4 bytes: 8 KB at q = 256 and degree 8, the largest this programme runs (nbl_create_fht32 refuses a larger check)
	const size_t lds = nbl_fht32_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (g.maxdc > NBL_MAXDC || lds > 64 * 1024 || blocks > 0x7fffffffLL || !f.v2c || !f.c2v) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_FHT32_Q(g.q, {
		if (g.maxdc <= 4) cn_fht32_kernel<QQ, 4><<<grid, block, lds, st>>>(g, w, f, r);
		else cn_fht32_kernel<QQ, NBL_MAXDC><<<grid, block, lds, st>>>(g, w, f, r);
	})
	return hipGetLastError();
}

hipError_t nbl_launch_cn_fht32_layered(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, const NblLayerDev &ly, int offset, int count,
                                       hipStream_t st)
{
	const size_t lds = nbl_fht32_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (count < 1 || offset < 0 || offset + count > g.M || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (g.maxdc > NBL_MAXDC || lds > 64 * 1024 || !f.v2c || !f.c2v || !f.Lf) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_FHT32_Q(g.q, {
		if (g.maxdc <= 4) cn_fht32_layered_kernel<QQ, 4><<<grid, block, lds, st>>>(g, w, f, r, ly, offset, count);
		else cn_fht32_layered_kernel<QQ, NBL_MAXDC><<<grid, block, lds, st>>>(g, w, f, r, ly, offset, count);
	})
	return hipGetLastError();
}
