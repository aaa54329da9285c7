// nbldpc_amd/csrc/nbl_soft.hip -- bit <-> symbol LLR conversion around the message-passing core (include/nbldpc.h: nbl_decode_batch_bits,
// nbl_soft_output).
//
//   bits_to_lch_kernel   per-bit LLRs [B][N p] -> the padded L_ch [B][N][q] of the workspace: the reference's RX_LLR_BIT -> RX_LLR_SYM
//                        loop (Comm.cpp:359-373), accumulated from 0.0 in ascending bit order
//   soft_output_kernel   the a-posteriori vector P[n] = L_ch[n] + c2v of n's edges (vn_decide_kernel's loads and sums, the same order) of
//                        the LAST decode call, written out unpadded, and its p bit marginals (max-log, or log-sum-exp); the EXT
//                        instances (NBL_SOFT_EXTRINSIC) start P[n] from 0.0 and never load L_ch
//
// The soft-output pass is one wave per (codeword, variable) at EVERY q, also where q < 64 leaves lanes idle.  That is deliberate: the
// pass runs once per decode call, not once per iteration, its cost is the one read of L_ch and c2v either way, and one variable per wave
// keeps every reduction a plain wave reduction.  Packing 64 / q variables into a wave would buy nothing that shows in a decode and would
// need segmented reductions: do not "fix" it.
//
// Which c2v buffer a codeword's messages are in is decided here, per codeword (NblSoftSrc), by the rule nbl_read_state applies on the
// host: everything the choice needs (done, iters) is already on the device, so the device entry point needs no host round trip.
#include <hip/hip_runtime.h>
#include "../../include/nbldpc.h"
#include "nbl_device.h"
#include "nbl_kernels.h"

// ---------------------------------------------------------------------------------------------------------
// bit LLRs -> L_ch.  Flat grid-stride over the B N q slots; consecutive lanes take consecutive a, so the stores coalesce at every q; the
// up to p lam values of a variable are the same addresses for all lanes of that variable (broadcast loads; scalar loads in the q >= 64
// instance, where a wave holds one variable: as vector loads they, not the stores, set the kernel's time -- DESIGN.md section 5h).
// Slot 0 gets the 0.0 the accumulation starts from.
// ---------------------------------------------------------------------------------------------------------
template <bool UNI> // UNI: q >= 64
__global__ __launch_bounds__(256) void bits_to_lch_kernel(const double *__restrict__ lam, double *__restrict__ Lch, long long total, int q, int p)
{
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const int a = (int)(i & (q - 1));
		long long bn = i >> p; // (q = 2^p: the (codeword, variable) index)
		// q >= 64: the 64 slots of a wave belong to ONE variable (the wave's first slot is a multiple of 64); saying so lets the p
		// values come through the scalar cache instead of as p vector loads whose lanes all read one address
		if (UNI) bn = ((long long)uniform((int)(bn >> 32)) << 32) | (unsigned)uniform((int)bn);
		const double *l = lam + bn * p;
		double v[8]; // all p values first (independent loads, the same for the q lanes of a variable), then the adds in ascending j
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = (j < p) ? l[j] : 0.0;
		double s = 0.0;
#pragma unroll
		for (int j = 0; j < 8; j++)
			if ((a >> j) & 1) s = s + v[j]; // (a < 2^p: no bit at or above p is set)
		Lch[i] = s;
	}
}

hipError_t nbl_launch_bits_to_lch(const double *d_lam, const NblGraphDev &g, const NblWork &w, int B, hipStream_t st)
{
	const long long total = (long long)B * g.N * g.q;
	long long blocks = (total + 255) / 256;
	if (blocks > 16384) blocks = 16384;
	if (blocks < 1) blocks = 1;
	if (g.q >= 64) bits_to_lch_kernel<true><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(d_lam, w.Lch, total, g.q, g.p);
	else bits_to_lch_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(d_lam, w.Lch, total, g.q, g.p);
	return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// soft output
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
	return v;
}

template <int Q, bool EXT = false>
__global__ __launch_bounds__(256) void soft_output_kernel(NblGraphDev g, const double *__restrict__ Lch, NblSoftSrc s, int B, int metric,
                                                          double *__restrict__ sym_llr, double *__restrict__ bit_llr)
{
	constexpr int NS = Fld<Q>::NS, P = Fld<Q>::P;
	const int lane = lane_id();
	const long long node = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (node >= (long long)B * g.N) return;
	const int b = (int)(node / g.N), n = (int)(node % g.N);

	// the codeword's c2v: as the last launched iteration left them, unless the codeword stopped earlier on the double-buffered path --
	// then the buffer iteration iters - 1 wrote (iteration i writes bufB when i is odd), the shared zero block for iters == 1
	const double *C;
	if (s.per_codeword && s.done[b]) {
		const int it = s.iters[b];
		C = (it == 1 && s.zeros) ? s.zeros : (((it - 1) & 1) ? s.bufB : s.bufA) + (size_t)b * g.E * Q;
	} else {
		C = s.last_shared ? s.last : s.last + (size_t)b * g.E * Q;
	}

	const int e0 = g.voff[n], dv = g.voff[n + 1] - e0;
	const double *L = Lch + ((size_t)b * g.N + n) * Q;
	double post[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) {
		const int a = lane + 64 * i;
		if constexpr (EXT) post[i] = 0.0;
		else post[i] = (a < Q) ? L[a] : 0.0;
	}
	for (int d = 0; d < dv; d++) {
		const double *Cd = C + (size_t)g.v_cpos[e0 + d] * Q;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			const int a = lane + 64 * i;
			if (a < Q) post[i] = post[i] + Cd[a];
		}
	}
	if (sym_llr) {
		double *S = sym_llr + ((size_t)b * g.N + n) * (Q - 1);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			const int a = lane + 64 * i;
			if (a >= 1 && a < Q) S[a - 1] = post[i];
		}
	}
	if (!bit_llr) return;

	// bit marginals.  Slot 0 holds P[0] = 0.0 (L_ch's slot 0 is 0.0 and so is every c2v's), so it counts in S0 with that value by
	// being a symbol like any other; lanes past the field (q < 64) are neutral: -inf for the maxima, 0 for the sums.
	double mine = 0.0;
#pragma unroll
	for (int j = 0; j < P; j++) {
		double m1 = NBL_NEG_INF, m0 = NBL_NEG_INF;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			const int a = lane + 64 * i;
			if (a < Q) {
				if ((a >> j) & 1) m1 = dmax(m1, post[i]);
				else m0 = dmax(m0, post[i]);
			}
		}
		// exact maxima: FP64 values on the DPP network (a float maximum would not be the maximum)
		const double M1 = wave_fmax(m1), M0 = wave_fmax(m0);
		double r;
		if (metric == NBL_SOFT_MAXLOG) {
			r = M1 - M0;
		} else {
			double s1 = 0.0, s0 = 0.0;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				const int a = lane + 64 * i;
				if (a < Q) {
					if ((a >> j) & 1) s1 = s1 + exp(post[i] - M1);
					else s0 = s0 + exp(post[i] - M0);
				}
			}
			s1 = wave_sum(s1);
			s0 = wave_sum(s0);
			r = (M1 + log(s1)) - (M0 + log(s0));
		}
		if (lane == j) mine = r + 0.0; // (a zero difference is +0.0 whatever the signs of the two zeros)
	}
	if (lane < P) bit_llr[((size_t)b * g.N + n) * P + lane] = mine;
}

hipError_t nbl_launch_soft_output(const NblGraphDev &g, const double *d_Lch, const NblSoftSrc &src, int B, int metric, double *d_sym_llr,
                                  double *d_bit_llr, hipStream_t st, bool extrinsic)
{
	const long long nodes = (long long)B * g.N, blocks = (nodes + 3) / 4;
	if (B < 1 || blocks > 0x7fffffffLL || !src.last || (src.per_codeword && (!src.bufA || !src.bufB || !src.done || !src.iters))) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(256);
	if (extrinsic) {
		NBL_DISPATCH_Q(g.q, soft_output_kernel<QQ, true><<<grid, block, 0, st>>>(g, d_Lch, src, B, metric, d_sym_llr, d_bit_llr))
	} else {
		NBL_DISPATCH_Q(g.q, soft_output_kernel<QQ><<<grid, block, 0, st>>>(g, d_Lch, src, B, metric, d_sym_llr, d_bit_llr))
	}
	return hipGetLastError();
}
