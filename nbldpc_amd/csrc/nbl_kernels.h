// nbldpc_amd/csrc/nbl_kernels.h -- host-callable launchers of nbl_kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_common.h"
#include "nbl_plan.h" // the nbl_*_applicable predicates, defined beside their kernels

// dynamic LDS of one workgroup on gfx950: what a kernel gets without opting in, and the ceiling every creation entry refuses above
// (pure arithmetic, before the device); the launch helper of nbl_cn_shell.h opts in between the two
#define NBL_LDS_OPT_IN (64 * 1024)
#define NBL_MAX_LDS (160 * 1024)

// inside a launcher: the statement(s) once per field size, with QQ = q as a constant; any other q returns hipErrorInvalidValue
#define NBL_DISPATCH_Q(q, ...)                                  \
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

hipError_t nbl_launch_init(const double *d_Lin, const NblGraphDev &g, const NblWork &w, int B, int write_v2c, hipStream_t st);
hipError_t nbl_launch_demod(const double *d_rx, int L, double sigma, int mod_order, const double *d_cons, const int *d_src,
                            const NblGraphDev &g, const NblWork &w, int B, hipStream_t st,
                            const double *d_gain = nullptr /* [B][L][2]: the gain-aware instance */);
// general demodulator, any mod_order = 2^m <= 256 (nbl_demod.hip); metric: NBL_DEMOD_* of include/nbldpc.h
hipError_t nbl_launch_demod_general(const double *d_rx, int L, double sigma, int mod_order, int metric, const double *d_cons,
                                    const NblDemodPoint *d_desc, const NblGraphDev &g, const NblWork &w, int B, hipStream_t st,
                                    const double *d_prior = nullptr /* [B][N p]: the prior-aware instance */, const int *d_tinv = nullptr,
                                    const double *d_gain = nullptr /* [B][L][2]: the gain-aware instances */);
hipError_t nbl_launch_vn(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool damp, hipStream_t st);
hipError_t nbl_launch_syn(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_compact(const uint8_t *done, int B, int *active, int *n_act, hipStream_t st);
hipError_t nbl_launch_cn_ems(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_unpad(const double *src, double *dst, const int *map, int rows, int q, hipStream_t st);
// general EMS kernel: deviation-count layers, and the bytes of LDS of one check (pure arithmetic: nbl_create refuses above NBL_MAX_LDS)
int nbl_ems_layers(int maxdc, int nc);
size_t nbl_ems_lds_bytes(int q, int maxdc, int nm, int nc);

// layered schedule for EMS (nbl_cn_layered.hip): decision + posterior without the v2c write, and the checks of one layer
// (chk[offset] .. chk[offset + count - 1]), inputs formed from L_ch and the in-place c2v
hipError_t nbl_launch_vn_decide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_ems_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// damped layered schedule for T-EMS (nbl_cn_tems_layered.hip): the checks of one layer; each forms its inputs from L_ch and the in-place
// c2v, damps them against the edge's stored v2c (w.v2c, updated in place) and runs the programme of nbl_cn_tems_core.h.  LDS: the
// larger of the two programmes a launch may take (pure arithmetic: nbl_create_layered_ex refuses above NBL_MAX_LDS before the device)
size_t nbl_tems_layered_lds_bytes(int q, int maxdc, int nc);
hipError_t nbl_launch_cn_tems_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// damped layered schedule for log-QSPA (nbl_cn_bp_layered.hip): the checks of one layer; inputs formed and damped as for T-EMS (0.5 / 0.5),
// then the programme of nbl_cn_bp_core.h.  LDS: (3 maxdc + 5) q 8 bytes, at most 59,392 B for the shapes the ABI accepts
hipError_t nbl_launch_cn_bp_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// FHT sum-product check node (nbl_create_fht; nbl_cn_fht.hip flooding, nbl_cn_fht_layered.hip the checks of one layer): the programme of
// nbl_cn_fht_core.h on the inputs of nbl_cn_bp_inputs.h, checks up to degree NBL_MAXDC.  LDS: maxdc q 8 bytes, at most 16 KB
hipError_t nbl_launch_cn_fht(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_fht_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);
// the same programme in the degree-independent layout of nbl_cn_fht_wide_core.h (nbl_cn_fht_wide.hip), checks up to degree
// NBL_FHT_MAX_CHECK_DEGREE.  LDS: maxdc q 8 bytes, at most 64 KB; the check's c2v region holds its forward products until the final store
hipError_t nbl_launch_cn_fht_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_fht_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// single-precision FHT decoding (nbl_create_fht32).  nbl_cn_fht32.hip: the programme of nbl_cn_fht32_core.h on the float state `f`,
// flooding and the checks of one layer, checks up to degree NBL_MAXDC; LDS: maxdc q 4 bytes, at most 8 KB.  nbl_fht32.hip: Lf = (float)
// L_ch with the initial v2c = Lf and c2v = 0 (one launch per decode call); the float variable-node pass (write_v2c: with the damped v2c
// half, the flooding schedule; without it, the decision pass of the layered schedule); dst[i] = (double) src[i], i < n
hipError_t nbl_launch_cn_fht32(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_fht32_layered(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, const NblLayerDev &ly, int offset, int count,
                                       hipStream_t st);
// the same with step 3a (every transformed input scaled by a power of two: nbl_cn_fht32_wide_core.h) in the degree-independent layout
// (nbl_cn_fht32_wide.hip; nbl_create_fht32_wide), checks up to degree NBL_FHT32_MAX_CHECK_DEGREE.  LDS: maxdc q 4 bytes, at most 32 KB; the
// check's float c2v region holds its forward products until the final store
hipError_t nbl_launch_cn_fht32_wide(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_fht32_wide_layered(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, const NblLayerDev &ly, int offset, int count,
                                            hipStream_t st);
hipError_t nbl_launch_narrow32(const NblGraphDev &g, const double *d_Lch, const NblWork32 &f, int B, hipStream_t st);
hipError_t nbl_launch_vn32(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, bool write_v2c, hipStream_t st);
hipError_t nbl_launch_widen32(const float *src, double *dst, long long n, hipStream_t st);

// EMS check node for checks up to degree NBL_EMS_MAX_CHECK_DEGREE (nbl_create_ems_wide; nbl_cn_ems_wide.hip): the programme of
// nbl_cn_ems_wide_core.h, one check per workgroup of max(1, q / 64) waves, flooding and the checks of one layer.  The bytes of LDS of one
// workgroup are pure arithmetic: nbl_create_ems_wide refuses above NBL_MAX_LDS before the device, both launchers size by it
size_t nbl_ems_wide_lds_bytes(int q, int maxdc, int nm, int nc);
hipError_t nbl_launch_cn_ems_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_ems_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// T-EMS check node for checks up to degree NBL_TEMS_MAX_CHECK_DEGREE over any field (nbl_create_tems_wide; nbl_cn_tems_wide.hip): the
// programme of nbl_cn_tems_wide_core.h, one check per workgroup of max(1, q / 64) waves, at most NBL_TEMS_WIDE_MAX_NC (nbl_tems_path.h)
// deviations per path, flooding and the checks of one layer.  The bytes of LDS of one workgroup are pure arithmetic:
// nbl_create_tems_wide refuses above NBL_MAX_LDS before the device, both launchers size by it
size_t nbl_tems_wide_lds_bytes(int q, int maxdc, int nr, int nc);
hipError_t nbl_launch_cn_tems_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_tems_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// exact log-QSPA check node for checks up to degree NBL_BP_MAX_CHECK_DEGREE (nbl_create_bp_wide; nbl_cn_bp_wide.hip): the programme of
// nbl_cn_bp_wide_core.h, one check per workgroup of max(1, q / 64) waves, flooding and the checks of one layer.  LDS of one workgroup:
// (maxdc + 5) q 8 + 256 bytes, at most 76,032 B (q = 256, degree 32) -- below NBL_MAX_LDS for every shape the ABI accepts, so
// nbl_create_bp_wide refuses no shape for LDS; both launchers size by the one function and check the bound all the same
size_t nbl_bp_wide_lds_bytes(int q, int maxdc);
hipError_t nbl_launch_cn_bp_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_bp_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// Min-Max check node (method 3; nbl_create_minmax; nbl_cn_minmax.hip): the programme of nbl_cn_minmax_core.h, one check per workgroup of
// max(1, q / 64) waves, check degrees up to NBL_MINMAX_MAX_CHECK_DEGREE, flooding (inputs: w.v2c) and the checks of one layer (inputs:
// L_ch and the in-place c2v).  LDS of one workgroup: (maxdc + 4) q 8 bytes, at most 73,728 B (q = 256, degree 32) -- below
// NBL_MAX_LDS for every shape the ABI accepts, so nbl_create_minmax refuses no shape for LDS; both launchers size by the one
// function and check the bound all the same
size_t nbl_minmax_lds_bytes(int q, int maxdc);
hipError_t nbl_launch_cn_minmax(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
hipError_t nbl_launch_cn_minmax_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st);

// specialised EMS check node (nbl_cn_ems256.hip)
size_t nbl_ems256_lds_bytes(int nm);
hipError_t nbl_launch_cn_ems256(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);

// T-EMS and log-QSPA check nodes (nbl_cn_tems.hip, nbl_cn_bp.hip)
hipError_t nbl_launch_cn_tems(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);
bool nbl_tems_use_fast(int nc); // the fast programme (nc <= 3) unless NBL_TEMS_GENERIC is set (A/B runs)
hipError_t nbl_launch_cn_bp(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);

// small fields (q <= 32; log-QSPA also q = 64), 64 / q checks per wave (nbl_cn_small.hip); method as in include/nbldpc.h (1 BP, 2 EMS, 4 T-EMS)
hipError_t nbl_launch_cn_ems_small(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);
hipError_t nbl_launch_cn_tems_small(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);
hipError_t nbl_launch_cn_bp_small(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);

// T-EMS check node for GF(64), check degree 4 (nbl_cn_tems64.hip)
hipError_t nbl_launch_cn_tems64(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);

// T-EMS check node for GF(256), check degree 4 (nbl_cn_tems256.hip)
hipError_t nbl_launch_cn_tems256(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);

// basic-set T-EMS check node, any q = 4 .. 256, check degree <= 8, 1 <= nm <= min(q - 1, 16) (nbl_cn_bstems.hip)
bool nbl_bstems_applicable(const NblGraphDev &g, int nm, int nc);
size_t nbl_bstems_lds_bytes(const NblGraphDev &g);
hipError_t nbl_launch_cn_bstems(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st);

// log-QSPA check node for GF(256), check degree 4 (nbl_cn_bp256.hip)
hipError_t nbl_launch_cn_bp256(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);

// EMS check node for GF(64): four checks per wave, four symbols per lane (nbl_cn_ems64.hip)
hipError_t nbl_launch_cn_ems64(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);

// log-QSPA check node for GF(64), check degree 4: four checks per wave, four symbols per lane (nbl_cn_bp64.hip)
hipError_t nbl_launch_cn_bp64(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool fused, hipStream_t st);

// bit <-> symbol LLR conversion around the iterations (nbl_soft.hip): per-bit LLRs [B][N p] -> w.Lch; and the a-posteriori vectors of
// the last decode call, unpadded [B][N][q-1], with their bit marginals [B][N p] (metric: NBL_SOFT_* of include/nbldpc.h; either output
// may be NULL)
hipError_t nbl_launch_bits_to_lch(const double *d_lam, const NblGraphDev &g, const NblWork &w, int B, hipStream_t st);
hipError_t nbl_launch_soft_output(const NblGraphDev &g, const double *d_Lch, const NblSoftSrc &src, int B, int metric, double *d_sym_llr,
                                  double *d_bit_llr, hipStream_t st, bool extrinsic = false /* NBL_SOFT_EXTRINSIC: P starts from 0.0 */);
// iterative demapping (nbl_idd.hip): results of a pass to the batch positions of its codewords; the survivors' rows to dense buffers
hipError_t nbl_launch_idd_scatter(const int *d_out, const uint8_t *d_done, const int *d_iters, const int *d_idx /* NULL: the identity */,
                                  int n, int N, int pass, int *d_res_out, uint8_t *d_res_done, int *d_res_iters, int *d_res_pass, hipStream_t st);
hipError_t nbl_launch_idd_gather(const int *d_active, int n, const double *d_rx_src, int rx_row, const double *d_ext_src, int prior_row,
                                 const int *d_idx_src /* NULL: the identity */, double *d_rx_dst, double *d_prior_dst, int *d_idx_dst,
                                 hipStream_t st, const double *d_gain_src = nullptr /* rows of rx_row doubles, carried like the samples */,
                                 double *d_gain_dst = nullptr);

// AWGN channel + CRand on the device (nbl_noise.hip)
hipError_t nbl_launch_noise_gen(const uint32_t *state, const uint32_t *jump, int L, int B, double *fn, uint32_t *flag_idx, double *flag_arg,
                                unsigned *flag_count, unsigned cap, hipStream_t st);
hipError_t nbl_launch_noise_patch(double *fn, const uint32_t *flag_idx, const double *val, unsigned n, hipStream_t st);
hipError_t nbl_launch_noise_finish(const double *fn, const uint8_t *tx_index, const double *cons, double sigma, int L, int B, double *rx, hipStream_t st);

// Rayleigh block fading on the device (nbl_fading.hip): fn [B][npos][2] double2 as nbl_launch_noise_gen leaves it over npos = nblk + L
// positions (the nblk gain draws first, then the L noise draws); RX = h * TX + noise and the per-sample gains
hipError_t nbl_launch_fading_finish(const double *fn, const uint8_t *tx_index, const double *cons, double sigma, int L, int nblk, int coherence,
                                    int B, double *rx, double *gain, hipStream_t st);

// transmit chain and error count on the device (nbl_tx.hip).  T is word-major: T[w * rows + r] = columns 64 w .. 64 w + 63 of row r.
#define NBL_TX_F 8 // frames a thread of the encode kernel carries (their packed inputs sit in LDS: NBL_TX_F * nw * 8 bytes)
hipError_t nbl_launch_tx_pn(const uint16_t *pn_state, const int16_t *phase_of, const uint8_t *seq, int period, int par_mod, int nb, int nw,
                            int B, unsigned long long *u, hipStream_t st);
hipError_t nbl_launch_tx_encode(const unsigned long long *T, const unsigned long long *u, int rows, int nw, int B, uint8_t *bits, hipStream_t st);
hipError_t nbl_launch_tx_pack(const uint8_t *bits, const int *keep, int N, int p, int L, int mb, int B, uint8_t *code, uint8_t *txi, hipStream_t st);
hipError_t nbl_launch_tx_msgbits(const int *msg, int K, int p, int nw, int B, unsigned long long *u, hipStream_t st);
hipError_t nbl_launch_tx_errcount(const int *dec, const uint8_t *code, const uint32_t *crc_col, int N, int K, int p, int crc_len, int B,
                                  int *err_sym, int *err_bit, uint8_t *crc_ok, hipStream_t st);
