// nbldpc_amd/csrc/nbl_osd.h -- ordered-statistics decoding on the device (nbl_osd.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_common.h"
#include "../../include/nbldpc.h"

struct NblOsdDev {
	const uint64_t *H; // [R][nw] [CRC rows; H_bit] bit-packed, nw = ceil(N p / 64), built at creation
	int R;             // crc_rows + M p
	int n_dist;        // positions the distance covers: (int)(N * log(q) / log(2)) as the reference computes it (host libm)
	int order, flag;   // order after the method-6 rule (>= 0); flag 1: L_ch, 0: S
	const double *S;   // flag 0: [B][N p] factor-weighted posterior sums (osd_acc_kernel)
};

#define NBL_OSD_MAX_LDS (160 * 1024) // LDS of one workgroup on gfx950
size_t nbl_osd_lds_bytes(int n, int R);
// one workgroup per codeword; codewords whose done flag is set are left alone
hipError_t nbl_launch_osd(const NblGraphDev &g, const NblWork &w, const NblOsdDev &o, int B, hipStream_t st);
// S[b][n p + k] = factor * S (0 when `first`) + post[b][n][2^k]
hipError_t nbl_launch_osd_acc(const double *post, double *S, int B, int N, int p, int q, double factor, int first, hipStream_t st);
