// nbldpc_amd/csrc/nbl_cn_bp_layered.hip -- log-QSPA under the damped layered (check-serial) schedule of include/nbldpc.h
// (nbl_create_layered_bp).
//
// One iteration is: vn_decide_kernel and syn_kernel (as for layered EMS and T-EMS), then ONE launch of cn_bp_layered_kernel per layer.
// A check of layer l forms the raw input of each of its edges from L_ch and the c2v buffer as the layers before it left it, damps it
// against the edge's stored v2c vector (the reference's per-edge damping, NBLDPC.cpp:730-741: where the hard decisions of the two
// differ, 0.5 old + 0.5 new), stores the result back as the edge's v2c, runs the log-QSPA check-node programme of the general kernel
// (nbl_cn_bp_core.h: the same device code) on it and writes its c2v vectors back into the same buffer.
//
// What makes one c2v and one v2c buffer enough:
//   * every global read of a check's inputs (L_ch, the neighbours' c2v, its own c2v, its stored v2c) happens in the first step of the
//     programme, which moves all dc inputs into LDS before its first convolution, and is complete before the check's first c2v store
//     in the programme's last step;
//   * the checks of a layer share no variable, so no wave of a launch reads a c2v vector that another wave of that launch writes;
//   * an edge belongs to one check, so its v2c vector is read and written by that check's wave alone;
//   * the launches of one stream order the layers.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_bp_core.h"
#include "nbl_cn_bp_inputs.h"

// the checks of one layer: one wave per (codeword, check); grid = count * (codeword slots)
template <int Q>
__global__ __launch_bounds__(64) void cn_bp_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int lane = lane_id();
	const int b = nbl_codeword(w, r, blockIdx.x / count), m = ly.chk[offset + blockIdx.x % count];
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const double *L = w.Lch + (size_t)b * g.N * Q;
	double *Cb = w.c2v + (size_t)b * g.E * Q;
	double *Vb = w.v2c + (size_t)b * g.E * Q;
	// (the input former of the damped layered schedule: nbl_cn_bp_inputs.h, shared with nbl_cn_fht_layered.hip)
	const BpLayeredInput<Q> input = {L, Cb, Vb, ly.nbr, g.c_epos, c0, lane, r.damp_old, r.damp_new};
	bp_check_node<Q>(g, smem, c0, dc, Cb + (size_t)c0 * Q, input);
}

#define NBL_LAYERED_Q(q, ...)                                   \
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

hipError_t nbl_launch_cn_bp_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	// (3 maxdc + 5) q 8 bytes: 59,392 B at q = 256 and degree 8, the largest the ABI accepts -- below the 64 KB a kernel has unasked
	const size_t lds = nbl_bp_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (count < 1 || offset < 0 || offset + count > g.M || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (lds > 64 * 1024) return hipErrorInvalidValue;
	if (!w.v2c) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_LAYERED_Q(g.q, { cn_bp_layered_kernel<QQ><<<grid, block, lds, st>>>(g, w, r, ly, offset, count); })
	return hipGetLastError();
}
