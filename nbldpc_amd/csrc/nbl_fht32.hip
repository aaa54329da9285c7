// nbldpc_amd/csrc/nbl_fht32.hip -- what single-precision FHT decoding (nbl_create_fht32) runs around its check node
// (nbl_cn_fht32.hip): the narrowing of the FP64 channel vectors, the float variable-node pass of the flooding schedule, the float
// decision pass of the layered schedule, and the widening of the float state for its FP64 readers.  The passes are those of
// nbl_kernels.hip / nbl_cn_layered.hip in IEEE binary32: the same sums in the same order, the same decision rule, the same damping;
// compiled with -ffp-contract=off.  The syndrome, compaction and output kernels read decisions only and are the FP64 kinds' own.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_fht32_core.h"

// ---------------------------------------------------------------------------------------------------------
// narrowing, once per decode call, after whichever front end filled the padded FP64 L_ch: Lf = (float) L_ch (round to nearest even),
// and the initial message state in the same launch: v2c of every edge of the variable = Lf, c2v = 0.  One wave per (codeword, variable).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void narrow32_kernel(NblGraphDev g, const double *__restrict__ Lch, NblWork32 f, int B)
{
	const int lane = lane_id(), q = g.q;
	const long long node = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (node >= (long long)B * g.N) return;
	const int b = (int)(node / g.N), n = (int)(node % g.N);
	const int e0 = g.voff[n], dv = g.voff[n + 1] - e0;
	const double *L = Lch + (size_t)node * q;
	float *Lf = f.Lf + (size_t)node * q;
	float *V = f.v2c + ((size_t)b * g.E + e0) * q;
	float *C = f.c2v + (size_t)b * g.E * q;
	for (int a = lane; a < q; a += 64) {
		const float x = a ? __double2float_rn(L[a]) : 0.0f;
		Lf[a] = x;
		for (int d = 0; d < dv; d++) {
			V[(size_t)d * q + a] = x;
			C[(size_t)g.v_cpos[e0 + d] * q + a] = 0.0f;
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// variable node, flooding: post = Lf + c2v_0 + c2v_1 ... (in that order), decision, v2c = post - c2v, damped 0.5 / 0.5 against the
// stored v2c where the two decide differently (vn_kernel<Q, true> of nbl_kernels.hip on floats)
// ---------------------------------------------------------------------------------------------------------
template <int Q, bool V2C>
__global__ __launch_bounds__(256) void vn32_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r)
{
	constexpr int NS = Fld<Q>::NS;
	const int lane = lane_id();
	const long long node = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (node >= (long long)r.B * g.N) return;
	const int b = nbl_codeword(w, r, (int)(node / g.N)), n = (int)(node % g.N);
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;

	const int e0 = g.voff[n], dv = g.voff[n + 1] - e0;
	const float *L = f.Lf + ((size_t)b * g.N + n) * Q;
	const float *C = f.c2v + (size_t)b * g.E * Q;

	float post[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) {
		int a = lane + 64 * i;
		post[i] = (a < Q) ? L[a] : 0.0f;
	}
	for (int d = 0; d < dv; d++) {
		const float *Cd = C + (size_t)g.v_cpos[e0 + d] * Q;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) post[i] = post[i] + Cd[a];
		}
	}
	const int dec = wave_decide32<NS>(post, lane, Q);
	if (lane == 0) w.dec[(size_t)b * g.N + n] = dec;
	if (f.post) {
		float *P = f.post + ((size_t)b * g.N + n) * Q;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) P[a] = post[i];
		}
	}
	if constexpr (V2C) {
		float *V = f.v2c + ((size_t)b * g.E + e0) * Q;
		const float damp_old = (float)r.damp_old, damp_new = (float)r.damp_new;
		for (int d = 0; d < dv; d++) {
			const float *Cd = C + (size_t)g.v_cpos[e0 + d] * Q;
			float *Vd = V + (size_t)d * Q;
			float nv[NS], ov[NS];
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				nv[i] = (a < Q) ? post[i] - Cd[a] : 0.0f;
				ov[i] = (a < Q) ? Vd[a] : 0.0f;
			}
			const int before = wave_decide32<NS>(ov, lane, Q);
			const int after = wave_decide32<NS>(nv, lane, Q);
			if (before != after) {
#pragma unroll
				for (int i = 0; i < NS; i++) nv[i] = __fadd_rn(__fmul_rn(damp_old, ov[i]), __fmul_rn(damp_new, nv[i]));
			}
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				if (a < Q) Vd[a] = (a == 0) ? 0.0f : nv[i];
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// widening for the FP64 readers of the state (nbl_read_state, nbl_soft_output*, the demapping loop): dst = (double) src, exact
// ---------------------------------------------------------------------------------------------------------
__global__ void widen32_kernel(const float *__restrict__ src, double *__restrict__ dst, long long n)
{
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = (double)src[i];
}

hipError_t nbl_launch_narrow32(const NblGraphDev &g, const double *d_Lch, const NblWork32 &f, int B, hipStream_t st)
{
	const long long nodes = (long long)B * g.N, blocks = (nodes + 3) / 4;
	if (B < 1 || blocks > 0x7fffffffLL || !d_Lch || !f.Lf || !f.v2c || !f.c2v) return hipErrorInvalidValue;
	narrow32_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(g, d_Lch, f, B);
	return hipGetLastError();
}

hipError_t nbl_launch_vn32(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, bool write_v2c, hipStream_t st)
{
	const long long nodes = (long long)r.B * g.N, blocks = (nodes + 3) / 4;
	if (blocks > 0x7fffffffLL || !f.Lf || !f.c2v || (write_v2c && !f.v2c)) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(256);
	if (write_v2c) { NBL_DISPATCH_Q(g.q, vn32_kernel<QQ, true><<<grid, block, 0, st>>>(g, w, f, r)) }
	else { NBL_DISPATCH_Q(g.q, vn32_kernel<QQ, false><<<grid, block, 0, st>>>(g, w, f, r)) }
	return hipGetLastError();
}

hipError_t nbl_launch_widen32(const float *src, double *dst, long long n, hipStream_t st)
{
	if (n < 1 || !src || !dst) return hipErrorInvalidValue;
	const long long want = (n + 255) / 256;
	widen32_kernel<<<dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, st>>>(src, dst, n);
	return hipGetLastError();
}
