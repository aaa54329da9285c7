// nbldpc_amd/csrc/nbl_idd.hip -- the two data movers of the iterative-demapping loop (include/nbldpc.h: nbl_decode_batch_samples_idd;
// DESIGN.md section 5i).  A pass of the loop decodes a dense sub-batch: row i of the workspace holds the codeword whose batch position
// is idx[i] (the identity in pass 1).
//
//   idd_scatter_kernel   after a pass: out / done / iters of row i, and the pass number, to position idx[i] of the [B] result buffers
//   idd_gather_kernel    before the next pass: for the i-th entry j of the active list (the rows that did not converge, ascending),
//                        the samples, the extrinsic bit LLRs (the next prior) and the batch position of row j into row i of the next
//                        pass's buffers.  Source and destination never alias: the samples ping-pong between two buffers and the
//                        caller's (or a slot's) samples are only ever read.  GAIN (nbl_decode_batch_samples_idd_csi, a slot with
//                        gains): the survivors' channel gains, rows of the samples' length, travel with their samples.
// Both are flat grid-stride copies: consecutive lanes take consecutive elements of a row.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"

__global__ __launch_bounds__(256) void idd_scatter_kernel(const int *__restrict__ out, const uint8_t *__restrict__ done, const int *__restrict__ iters,
                                                          const int *__restrict__ idx, int n, int N, int pass, int *__restrict__ res_out,
                                                          uint8_t *__restrict__ res_done, int *__restrict__ res_iters, int *__restrict__ res_pass)
{
	const long long total = (long long)n * N;
	for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
		const int i = (int)(e / N), k = (int)(e % N);
		const int b = idx ? idx[i] : i;
		res_out[(size_t)b * N + k] = out[e];
		if (k == 0) {
			res_done[b] = done[i];
			res_iters[b] = iters[i];
			res_pass[b] = pass;
		}
	}
}

template <bool GAIN>
__global__ __launch_bounds__(256) void idd_gather_kernel(const int *__restrict__ active, int n, const double *__restrict__ rx_src, int rx_row,
                                                         const double *__restrict__ ext_src, int prior_row, const int *__restrict__ idx_src,
                                                         double *__restrict__ rx_dst, double *__restrict__ prior_dst, int *__restrict__ idx_dst,
                                                         const double *__restrict__ gain_src, double *__restrict__ gain_dst)
{
	const int row = rx_row + prior_row + (GAIN ? rx_row : 0);
	const long long total = (long long)n * row;
	for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
		const int i = (int)(e / row), k = (int)(e % row);
		const int j = active[i];
		if (k < rx_row) rx_dst[(size_t)i * rx_row + k] = rx_src[(size_t)j * rx_row + k];
		else if (k < rx_row + prior_row) prior_dst[(size_t)i * prior_row + (k - rx_row)] = ext_src[(size_t)j * prior_row + (k - rx_row)];
		else if constexpr (GAIN) gain_dst[(size_t)i * rx_row + (k - rx_row - prior_row)] = gain_src[(size_t)j * rx_row + (k - rx_row - prior_row)];
		if (k == 0) idx_dst[i] = idx_src ? idx_src[j] : j;
	}
}

static unsigned idd_blocks(long long total)
{
	long long blocks = (total + 255) / 256;
	if (blocks > 16384) blocks = 16384;
	return (unsigned)(blocks < 1 ? 1 : blocks);
}

hipError_t nbl_launch_idd_scatter(const int *d_out, const uint8_t *d_done, const int *d_iters, const int *d_idx, int n, int N, int pass,
                                  int *d_res_out, uint8_t *d_res_done, int *d_res_iters, int *d_res_pass, hipStream_t st)
{
	if (n < 1 || N < 1 || !d_out || !d_done || !d_iters || !d_res_out || !d_res_done || !d_res_iters || !d_res_pass) return hipErrorInvalidValue;
	idd_scatter_kernel<<<dim3(idd_blocks((long long)n * N)), dim3(256), 0, st>>>(d_out, d_done, d_iters, d_idx, n, N, pass, d_res_out, d_res_done,
	                                                                             d_res_iters, d_res_pass);
	return hipGetLastError();
}

hipError_t nbl_launch_idd_gather(const int *d_active, int n, const double *d_rx_src, int rx_row, const double *d_ext_src, int prior_row,
                                 const int *d_idx_src, double *d_rx_dst, double *d_prior_dst, int *d_idx_dst, hipStream_t st,
                                 const double *d_gain_src, double *d_gain_dst)
{
	if (n < 1 || rx_row < 1 || prior_row < 1 || !d_active || !d_rx_src || !d_ext_src || !d_rx_dst || !d_prior_dst || !d_idx_dst) return hipErrorInvalidValue;
	if ((d_gain_src == nullptr) != (d_gain_dst == nullptr)) return hipErrorInvalidValue;
	if (d_gain_src)
		idd_gather_kernel<true><<<dim3(idd_blocks((long long)n * (2 * rx_row + prior_row))), dim3(256), 0, st>>>(
		    d_active, n, d_rx_src, rx_row, d_ext_src, prior_row, d_idx_src, d_rx_dst, d_prior_dst, d_idx_dst, d_gain_src, d_gain_dst);
	else
		idd_gather_kernel<false><<<dim3(idd_blocks((long long)n * (rx_row + prior_row))), dim3(256), 0, st>>>(
		    d_active, n, d_rx_src, rx_row, d_ext_src, prior_row, d_idx_src, d_rx_dst, d_prior_dst, d_idx_dst, nullptr, nullptr);
	return hipGetLastError();
}
