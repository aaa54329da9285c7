// nbldpc_amd/csrc/nbl_cn_fht32_wide.hip -- single-precision FHT sum-product check node for checks of degree up to
// NBL_FHT32_MAX_CHECK_DEGREE (nbl_create_fht32_wide on a code with a check above degree 8, or any such decoder under
// nbl_debug_force_generic(dec, 3)): the programme of nbl_cn_fht32_wide_core.h, one instantiation per q for every degree, under both
// schedules.  The launch shapes and the input formers are those of nbl_cn_fht32.hip: one wave per (codeword, check); every global read of
// a check's inputs happens in the programme's first step; between that step and a c2v region's final store the region holds the check's
// forward product, which only the owning wave reads -- the checks of a layer share no variable, and the launches of a stream order
// everything else.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_fht32_wide_core.h"
#include "nbl_cn_fht32_inputs.h"

template <int Q>
__global__ __launch_bounds__(64) void cn_fht32_wide_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const Bp32V2cInput<Q> in = {f.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	fht32_wide_check_node<Q, Bp32V2cInput<Q>>(g, smem, c0, dc, f.c2v + ((size_t)b * g.E + c0) * Q, in);
}

// the checks of one layer: grid = count * (codeword slots)
template <int Q>
__global__ __launch_bounds__(64) void cn_fht32_wide_layered_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / count), m = ly.chk[offset + blockIdx.x % count];
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	float *Cb = f.c2v + (size_t)b * g.E * Q;
	const Bp32LayeredInput<Q> input = {f.Lf + (size_t)b * g.N * Q, Cb, f.v2c + (size_t)b * g.E * Q, ly.nbr, g.c_epos, c0, lane_id(), (float)r.damp_old, (float)r.damp_new};
	fht32_wide_check_node<Q, Bp32LayeredInput<Q>>(g, smem, c0, dc, Cb + (size_t)c0 * Q, input);
}

#define NBL_FHT32_WIDE_Q(q, ...)                                \
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

// maxdc q 4 bytes of LDS: 32 KB at q = 256 and degree 32, the largest nbl_create_fht32_wide accepts
static bool wide32_shape_ok(const NblGraphDev &g, const NblWork32 &f)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_FHT32_MAX_CHECK_DEGREE && nbl_fht32_wide_lds_bytes(g.q, g.maxdc) <= 64 * 1024 && f.v2c && f.c2v;
}

hipError_t nbl_launch_cn_fht32_wide(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_fht32_wide_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (!wide32_shape_ok(g, f) || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_FHT32_WIDE_Q(g.q, cn_fht32_wide_kernel<QQ><<<grid, block, lds, st>>>(g, w, f, r))
	return hipGetLastError();
}

hipError_t nbl_launch_cn_fht32_wide_layered(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, const NblLayerDev &ly, int offset, int count,
                                            hipStream_t st)
{
	const size_t lds = nbl_fht32_wide_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (count < 1 || offset < 0 || offset + count > g.M || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (!wide32_shape_ok(g, f) || !f.Lf) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_FHT32_WIDE_Q(g.q, cn_fht32_wide_layered_kernel<QQ><<<grid, block, lds, st>>>(g, w, f, r, ly, offset, count))
	return hipGetLastError();
}
