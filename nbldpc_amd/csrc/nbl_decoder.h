// nbldpc_amd/csrc/nbl_decoder.h -- private to the nbl_api*.cpp units: the decoder handle, the error macros and the few helpers one
// unit defines and another calls.
//   nbl_api_create.cpp   nbl_create* (argument checks, graph indices, layer assignment, uploads)
//   nbl_api.cpp          workspace, destroy, the iteration loop, nbl_decode_batch*, state read-back, debug switches
//   nbl_api_demod.cpp    nbl_set_demodulator*, samples / prior / csi decodes, bit-LLR input, soft output, iterative demapping
//   nbl_api_channel.cpp  nbl_rand_advance, the noise and fading channel, the resident slots, nbl_set_fading, channel diagnostics
//   nbl_api_tx.cpp       nbl_pn_advance, nbl_set_transmitter, transmit, error count, encode, the slot read-backs
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/nbldpc.h"
#include "nbl_buf.h"
#include "nbl_kernels.h"
#include "nbl_osd.h"

// (nothing declared here is part of the library's interface: it stays out of the dynamic symbol table)
#pragma GCC visibility push(hidden)

struct nbl_decoder {
	int device = -1;
	nbl_params prm{};
	nbl_params_ext ext{};       // method 7 only (nbl_create_ex)
	bool osd_on = false;        // OSD stage after the iterations (method 6, or order >= 0; nbl_create_osd)
	bool osd_acc = false;       // flag-0 posterior sums after every variable-node pass (needs w.post)
	NblOsdDev osd{};            // H uploaded at creation; S set per decode
	double osd_factor = 0.0;
	NblGraphDev g{};
	NblWork w{};                // the launchers' view of the workspace: raw pointers into `ws`, set by ensure_workspace
	std::vector<void *> graph_allocs;
	int *d_e2c_map = nullptr;   // variable-major edge -> check-major slot (same as v_cpos), for c2v read-back
	int cap = 0;                // codewords the workspace holds
	struct Ws {                 // the workspace: made together by ensure_workspace, dropped together by free_workspace
		DevBuf<double> Lch, v2c, c2v, post;
		DevBuf<int> dec, edge_dec, out, iters;
		DevBuf<uint8_t> done;
		DevBuf<double> c2v_alt;  // second c2v buffer of the fused EMS iteration (flooding schedule -> double buffer)
		DevBuf<double> c2v_zero; // fused iterations: the all-zero c2v of iteration 0, ONE [E][q] block shared by all codewords, written once
		                         // when the workspace is made and only ever read (iteration 1 reads it instead of a buffer that would
		                         // have to be cleared on every call)
		DevBuf<double> osd_S;    // [cap][N p]
		DevBuf<int> active;      // [cap] active list (early exit, batches of NBL_COMPACT_MIN codewords or more)
		DevBuf<double> Lin;      // staging of the host-layout input [cap][N][q-1], made by the first nbl_decode_batch: not counted
		// nbl_create_fht32 / nbl_create_fht32_wide: the float state the iterations run on (post32 only when state recording is on).  On such a decoder v2c, c2v
		// and post above are made by the first call that reads the state in FP64 (widen_state), not with the workspace
		DevBuf<float> Lf, v2c32, c2v32, post32;
		size_t bytes() const
		{
			return Lch.size + v2c.size + c2v.size + post.size + dec.size + edge_dec.size + out.size + iters.size + done.size + c2v_alt.size +
			       c2v_zero.size + osd_S.size + active.size + Lf.size + v2c32.size + c2v32.size + post32.size;
		}
	} ws;
	NblWork32 w32{};            // the float launchers' view of the workspace (nbl_kind_f32 decoders only)
	bool wide_valid = false;    // w.c2v / w.v2c / w.post hold the widening of the last decode's float state ...
	hipStream_t wide_stream = nullptr; // ... made on this stream
	hipStream_t stream = nullptr;
	bool record_state = false;
	NblShape shape{};           // what the kernel choice depends on (nbl_plan.h)
	const double *last_c2v = nullptr;
	bool last_fused = false;    // the last decode ran fused iterations (nbl_read_state picks the c2v buffer per codeword)
	// The check-node half of iteration max_iter, which only a reader of the message state needs (undamped fused EMS; DESIGN.md section
	// 4): the decode ran that iteration's variable-node pass alone (vn_decide on the c2v of iteration max_iter - 1) and left the fused
	// launch to finish_pending.  Dropped, not run, by the next decode and wherever the workspace or the graphs go.
	struct Pending {
		bool on = false;
		bool timed = false;           // the decode was profiled: nbl_last_timing counts the launches its times cover, not the owed pass
		bool foreign = false;         // the decode ran on a caller's stream: pending_ev marks its end there
		int iter = 0;                 // = max_iter
		const double *prev = nullptr; // c2v of iteration iter - 1 (read)
		double *out = nullptr;        // c2v of iteration iter (written)
		int batch = 0;
		NblCn cn{};
		NblRun r{};                   // as the skipped launch would have had it, B = batch
	} pending;
	hipEvent_t pending_ev = nullptr; // made by the first decode on a caller's stream that defers
	bool defer_last = true;          // nbl_debug_defer_last; NBL_DEFER_LAST=0 makes handles with it off
	// layered (check-serial) schedule (nbl_create_layered / nbl_create_layered_ex / nbl_create_layered_bp): one c2v buffer updated in
	// place; EMS keeps no v2c, T-EMS (NBL_LAYERED_DAMPED) and log-QSPA keep the per-edge v2c their damping reads, updated in place by the
	// edge's check
	bool layered = false;
	NblKind kind = NBL_KIND_BASE; // the entry point that made the handle (nbl_plan.h; flooding or layered, whichever kind)
	int n_layers = 0;
	std::vector<int> h_layer_of; // [M] the assignment in use
	std::vector<int> h_lay_off;  // [n_layers + 1] offsets into ly.chk
	NblLayerDev ly{};
	// device-side demodulator (nbl_set_demodulator)
	int dm_order = 0, dm_L = 0;
	DevBuf<double> d_cons;
	DevBuf<int> d_src;
	bool dm_general = false;           // the general kernel (nbl_demod.hip): d_dmdesc in place of d_src
	int dm_metric = 0;                 // NBL_DEMOD_*
	DevBuf<NblDemodPoint> d_dmdesc;    // [N][p + 1]
	DevBuf<double> d_rx;
	// iterative demapping (nbl_decode_batch_samples_prior / _idd)
	DevBuf<int> d_tinv;                // [L m] general path: the code bit that claims label bit t (the inverse of src), -1 = nobody
	DevBuf<double> d_prior;            // staging of a host prior [B][N p]; counted in nbl_workspace_bytes
	struct Idd {                       // buffers of the loop, grown on demand, counted in nbl_workspace_bytes
		DevBuf<double> rx[2];          // samples of the survivors, ping-pong (pass k reads one, the gather fills the other)
		DevBuf<double> gain[2];        // their channel gains, when the call has gains
		DevBuf<int> idx[2];            // their batch positions
		DevBuf<double> ext, prior;     // extrinsic bit LLRs of a pass [n][N p]; the survivors' rows of it = the next prior
		DevBuf<int> res_out, res_iters, res_pass; // [B][N], [B], [B]: results at batch positions
		DevBuf<uint8_t> res_done;
		size_t bytes() const
		{
			return rx[0].size + rx[1].size + gain[0].size + gain[1].size + idx[0].size + idx[1].size + ext.size + prior.size + res_out.size +
			       res_iters.size + res_pass.size + res_done.size;
		}
	} idd;
	// flat fading (nbl_set_fading, nbl_decode_batch_samples_csi)
	int fade_model = NBL_FADING_NONE, fade_coh = 1;
	DevBuf<uint32_t> d_jump_f;         // [3][nblk + L] A^(4 k) mod m: the fading frame's positions (gains, then noise)
	int jump_f_pos = 0;                // the position count d_jump_f was made for
	DevBuf<double> d_gain;             // [B][L][2] gains beside d_rx: staging of a host array, or what the channel of nbl_decode_batch_noise formed;
	                                   // counted in nbl_workspace_bytes
	bool rx_gain = false;              // d_gain holds the gains of the samples in d_rx
	DevBuf<double> d_gains[2];         // resident gains beside d_rxs, one per slot (filled on the channel thread); counted in nbl_workspace_bytes
	bool slot_gain[2] = {false, false};      // the slot's samples were formed under fading: its gains are valid
	bool idd_sub = false;              // the last decode call was a loop with passes > 1: the workspace holds its last sub-batch
	// bit-LLR input and soft output (nbl_decode_batch_bits, nbl_soft_output): staging of the host forms, grown on demand, counted in
	// nbl_workspace_bytes from the moment they exist
	DevBuf<double> d_lam, d_soft_sym, d_soft_bit;
	// device-side AWGN channel (nbl_decode_batch_noise)
	std::vector<double> h_cons;  // constellation as given to nbl_set_demodulator
	DevBuf<uint32_t> d_jump;     // [3][L] A^(4 s) mod m of the three generators
	DevBuf<unsigned> d_fcount;
	struct Noise {               // sized for noise_cap lanes of noise_pos positions, remade together when either grows
		DevBuf<uint32_t> state;  // [cap][3]
		DevBuf<uint8_t> txi;     // [cap][L]
		DevBuf<double> fn;       // [cap][L][2][2]: log(1 - u1), cos(2 pi u2) of every normal draw
		DevBuf<uint32_t> fidx;   // uncertain values: index into fn, argument, host-evaluated value
		DevBuf<double> farg, fval;
		HostBuf<double> h_farg, h_fval; // pinned host mirrors
	} noise;
	size_t noise_cap = 0, noise_pos = 0, flag_cap = 0;
	double last_flag_frac = 0.0;
	hipStream_t stream2 = nullptr; // the channel of batch k+1 runs here while batch k is decoded on `stream`
	DevBuf<double> d_rxs[2];       // resident received samples of nbl_channel_batch, one per slot
	int rxs_B[2] = {0, 0};
	// device-side transmitter and error count (nbl_set_transmitter); dropped as a whole by assigning Tx()
	struct Tx {
		bool on = false;
		int crc_len = 0, random_msg = 0, K = 0, nb = 0, nw = 0, nwg = 0, mb = 0, period = 1, par_mod = 0;
		DevBuf<unsigned long long> T;     // [nw][N p] PN bits -> code bits
		DevBuf<unsigned long long> G_crc; // [nwg][N p] message bits -> code bits, when crc_len != 0
		const unsigned long long *G = nullptr; // that matrix: T when crc_len == 0, else G_crc (NULL without a generator)
		DevBuf<int> keep;             // [L mb] code bit carried by every modulator bit
		DevBuf<uint32_t> crc_col;     // [K p] remainder of message bit i under CrcCheck's type-1 polynomial
		DevBuf<int16_t> phase_of;     // [2048] register state -> position in seq, -1 = all-zero output
		DevBuf<uint8_t> seq;          // [period] output bit of the register along its cycle
		DevBuf<uint16_t> pn;          // [B] staging of pn_state
		DevBuf<unsigned long long> u; // [B][nw]
		DevBuf<uint8_t> bits;         // [B][N p]
		DevBuf<uint8_t> code[2], txi[2]; // per slot: [B][N] code symbols, [B][L] constellation indices
		int tx_B[2] = {0, 0};
		DevBuf<int> dec[2];           // per slot: outputs of the last nbl_decode_batch_resident
		int dec_B[2] = {0, 0};
		DevBuf<int> cnt;              // [cnt_cap] err_sym, [cnt_cap] err_bit, then [cnt_cap] bytes crc_ok
		size_t cnt_cap = 0;
		// nbl_encode_batch scratch (decode thread)
		DevBuf<int> e_msg; DevBuf<unsigned long long> e_u; DevBuf<uint8_t> e_bits, e_code;
	} tx;
	std::string err2;              // error text of the channel thread (nbl_channel_batch); nbl_last_error reports both
	// hipGraph replay of the iteration loop: one executable graph per window of iterations (fixed iterations: the whole loop;
	// early exit: the `poll_every` iterations between two polls), captured on the decoder's own stream the first time a window is
	// run with a given set of buffers, replayed on the caller's stream afterwards.  NBL_GRAPH=0 switches it off.
	struct GraphKey { const void *lin, *lch, *v2c, *c2v, *alt, *post, *osd_s; int B, record, generic, fused; };
	GraphKey gkey{};
	std::vector<hipGraphExec_t> gexec; // index = window number
	bool use_compact = true;           // NBL_COMPACT=0 switches it off
	bool use_graph = false;            // opt-in (NBL_GRAPH=1): measured gain is nil, see DESIGN.md section 7
	int force_generic = 0;      // debug: 1 = always the generic kernels, 2 = specialised kernels but no VN/CN fusion
	bool profiling = false;
	hipEvent_t ev[2] = {nullptr, nullptr};
	HostBuf<int> h_ndone;        // pinned [2]: converged-codeword counts read back after each window of iterations
	std::vector<hipEvent_t> pev; // per-launch events (profiling only)
	double ms[4] = {0, 0, 0, 0};
	long long launches[3] = {0, 0, 0};
	int last_B = 0;
	std::vector<int> h_coff, h_cvar, h_ch; // check-major graph and the multiplication table on the host (nbl_set_transmitter: H gen = 0)
	std::vector<uint16_t> h_mul;
	std::string err;
};

// HIP_TRY_E: the failing call's text goes into `errstr` -- dec->err for everything the decode thread does, dec->err2 for the channel
// thread (nbl_channel_batch may run beside a decode on the same handle, so the two never share a string)
#define HIP_TRY_E(errstr, call)                                                                    \
	do {                                                                                           \
		hipError_t e_ = (call);                                                                    \
		if (e_ != hipSuccess) {                                                                    \
			(errstr) = std::string(#call) + ": " + hipGetErrorString(e_);                          \
			return NBL_ERR_HIP;                                                                    \
		}                                                                                          \
	} while (0)
#define HIP_TRY(dec, call) HIP_TRY_E((dec)->err, call)

static inline int ilog2(int q)
{
	int p = 0;
	while ((1 << p) < q) p++;
	return p;
}

// what nbl_soft_output and nbl_read_state refuse after a loop of several passes
inline const char *const NBL_IDD_SUB_TEXT = ": the last decode call was an iterative-demapping loop (passes > 1), the workspace holds the "
                                            "sub-batch of its last pass and not the batch; run an ordinary decode call first";

// nbl_api_create.cpp: one row per entry point beside nbl_create* / nbl_create_layered* -- what its wrapper, create_impl's method and
// degree checks and nbl_debug_plan_kind need to know of a kind
struct NblEntry {
	NblKind kind;
	const char *name, *fn;    // "fht" (nbl_debug_plan_kind's kind_name), "nbl_create_fht" (as the messages name it)
	uint32_t layered_bit;     // its one flag, NBL_*_LAYERED ...
	const char *layered_flag; // ... and that flag's name
	int method;               // the one method it runs
	const char *method_text;  // what follows `fn` in the refusal of any other
	int max_dc;               // the largest check degree it takes
	const char *max_dc_text;  // what follows "(max_dc)" in the refusal of a larger one
	uint32_t lay_flags;       // the layered schedule it runs: NBL_LAYERED_* of nbl_create_layered_ex ...
	bool lay_bp;              // ... or that of nbl_create_layered_bp
};
const NblEntry *nbl_entry(NblKind kind);            // NULL for NBL_KIND_BASE
const NblEntry *nbl_entry_named(const char *name);  // NULL for a name no row has

// nbl_api.cpp
extern thread_local std::string g_create_error; // what nbl_last_error(NULL) reports
nbl_status ensure_workspace(nbl_decoder *d, int B);
nbl_status run_iterations(nbl_decoder *d, const double *d_Lin, int B, hipStream_t st);
// Runs the deferred check-node pass of the last decode, if one is pending, on d->stream; every reader of the last c2v calls it first.
// reader: the stream that will read the c2v (NULL or d->stream: nothing more to order).
nbl_status finish_pending(nbl_decoder *d, hipStream_t reader = nullptr);
// nbl_create_fht32 / nbl_create_fht32_wide decoders (nothing to do on any other): the float post / c2v / v2c of the last decode call widened, exactly, into the
// FP64 w.post / w.c2v / w.v2c, which are made here the first time; every FP64 reader of the message state calls it first.  reader: the
// stream that will read (NULL: d->stream); the widening runs on it.
nbl_status widen_state(nbl_decoder *d, hipStream_t reader = nullptr);
// The results of a decode call, B codewords from out / done / iters (the workspace's, or the loop's at batch positions), to the
// caller's arrays on `st`; to_done and to_iters may be NULL.  sync: wait for the stream afterwards (the host forms).
nbl_status read_back(nbl_decoder *d, const int *out, const uint8_t *done, const int *iters, int B, int32_t *to_out, uint8_t *to_done,
                     int32_t *to_iters, hipMemcpyKind kind, hipStream_t st, bool sync);
// nbl_api_demod.cpp
hipError_t launch_demod(nbl_decoder *d, const double *d_rx, double sigma, int B, const double *d_prior = nullptr, const double *d_gain = nullptr);
nbl_status run_idd(nbl_decoder *d, const double *d_rx0, double sigma, int B, const nbl_idd_params *idd, const double *d_gain0 = nullptr);
// nbl_api_channel.cpp
nbl_status run_channel(nbl_decoder *d, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int B, hipStream_t st,
                       DevBuf<double> &rx_buf, DevBuf<double> &gain_buf, bool *has_gain, std::string &err, const uint8_t *d_txi_dev = nullptr);
nbl_status resident_check(nbl_decoder *d, int slot, int B, const int32_t *out_sym);

#pragma GCC visibility pop
