// nbldpc_amd/csrc/nbl_fading.hip -- Rayleigh block fading on the device (include/nbldpc.h, nbl_set_fading).
//
// A frame of a lane draws, in this order, two normals per block of `coherence` samples (the gain, sigma = sqrt(0.5) each) and then
// Channel_AWGN's two normals per sample.  Every normal is two uniform draws, so the frame is nblk + L POSITIONS of four uniform draws
// each, counted from the lane's state: the gains are the first nblk positions, the noise of sample s is position nblk + s -- the state
// moved on by 4 nblk draws.  nbl_noise.hip's noise_gen_kernel runs unchanged over those nblk + L positions (its jump table is per
// position count: A^(4 k) for k < nblk + L, kept beside the AWGN table of L positions), with its certainty verdicts and the host-libm
// patch list, so every log / cos equals glibc's bit for bit.  What is new is the last step:
//   fading_finish_kernel  one thread per sample: h_k = 0 + S * cs * sqrt(-2 lg) per component (Rand.cpp:35's order), the noise likewise
//                         with sigma, RX = (hr cr - hi ci, hr ci + hi cr) + (nr, ni) in the header's order, and the gain of the
//                         sample written beside it: gain[b][s] = h_(s / coherence)
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"

__global__ __launch_bounds__(256) void fading_finish_kernel(const double2 *__restrict__ fn, const uint8_t *__restrict__ tx_index,
                                                            const double *__restrict__ cons, double sigma, double S, double mu, int L, int nblk,
                                                            int coherence, long long nsym, double2 *__restrict__ rx, double2 *__restrict__ gain)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nsym) return;
	const long long b = i / L;
	const int s = (int)(i % L), k = s / coherence;
	const double2 *f = fn + (size_t)b * (size_t)(nblk + L) * 2; // this lane's positions: [nblk + L][2] (component)[lg, cs]
	const double2 gr = f[2 * k], gi = f[2 * k + 1];
	const double2 fr = f[2 * (size_t)(nblk + s)], fi = f[2 * (size_t)(nblk + s) + 1];
	// Rand_Norm: mu + sigma * cos(..) * sqrt(-2.0 * log(..)), left to right (Rand.cpp:35); mu = 0 arrives as an argument so that the
	// addition stays an addition
	const double hr = mu + S * gr.y * sqrt(-2.0 * gr.x);
	const double hi = mu + S * gi.y * sqrt(-2.0 * gi.x);
	const double nr = mu + sigma * fr.y * sqrt(-2.0 * fr.x);
	const double ni = mu + sigma * fi.y * sqrt(-2.0 * fi.x);
	const int t = tx_index[i];
	const double cr = cons[2 * t], ci = cons[2 * t + 1];
	double2 o, h;
	o.x = (hr * cr - hi * ci) + nr;
	o.y = (hr * ci + hi * cr) + ni;
	h.x = hr;
	h.y = hi;
	rx[i] = o;
	gain[i] = h;
}

hipError_t nbl_launch_fading_finish(const double *fn, const uint8_t *tx_index, const double *cons, double sigma, int L, int nblk, int coherence,
                                    int B, double *rx, double *gain, hipStream_t st)
{
	if (L < 1 || coherence < 1 || nblk != (L + coherence - 1) / coherence || !fn || !tx_index || !cons || !rx || !gain) return hipErrorInvalidValue;
	const long long nsym = (long long)B * L;
	fading_finish_kernel<<<dim3((unsigned)((nsym + 255) / 256)), dim3(256), 0, st>>>((const double2 *)fn, tx_index, cons, sigma, sqrt(0.5), 0.0, L, nblk,
	                                                                                coherence, nsym, (double2 *)rx, (double2 *)gain);
	return hipGetLastError();
}
