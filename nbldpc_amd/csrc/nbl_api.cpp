// nbldpc_amd/csrc/nbl_api.cpp -- C ABI (include/nbldpc.h) on top of the HIP kernels.
//
// Replaces CNBLDPC::Initial's decoder set-up (NBLDPC.cpp:140-377: graph cross indices, message buffers) and
// CNBLDPC::Decoding's iteration loop (NBLDPC.cpp:607-641 -> Decoding_BP/EMS/TEMS/BS_TEMS) for a batch of codewords.
// No CPU decode path exists in this library: without a HIP device nbl_create() fails.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <cmath>
#include <string>
#include <thread>
#include <vector>
#include "../../include/nbldpc.h"
#include "nbl_kernels.h"
#include "nbl_osd.h"

static thread_local std::string g_create_error;

struct nbl_decoder {
	int device = -1;
	nbl_params prm{};
	nbl_params_ext ext{};       // method 7 only (nbl_create_ex)
	bool osd_on = false;        // OSD stage after the iterations (method 6, or order >= 0; nbl_create_osd)
	bool osd_acc = false;       // flag-0 posterior sums after every variable-node pass (needs w.post)
	NblOsdDev osd{};            // H uploaded at creation; S set per decode
	double osd_factor = 0.0;
	double *osd_S = nullptr;    // [cap][N p]
	NblGraphDev g{};
	NblWork w{};
	std::vector<void *> graph_allocs;
	int *d_e2c_map = nullptr;   // variable-major edge -> check-major slot (same as v_cpos), for c2v read-back
	int cap = 0;                // codewords the workspace holds
	size_t ws_bytes = 0;
	double *d_Lin = nullptr;    // staging of the host-layout input [cap][N][q-1]
	uint8_t *d_conv8 = nullptr;
	hipStream_t stream = nullptr;
	bool record_state = false;
	NblShape shape{};           // what the kernel choice depends on (nbl_plan.h)
	double *c2v_alt = nullptr;  // second c2v buffer of the fused EMS iteration (flooding schedule -> double buffer)
	double *c2v_zero = nullptr; // fused iterations: the all-zero c2v of iteration 0, ONE [E][q] block shared by all codewords, written once
	                            // when the workspace is made and only ever read (iteration 1 reads it instead of a buffer that would
	                            // have to be cleared on every call)
	const double *last_c2v = nullptr;
	bool last_fused = false;    // the last decode ran fused iterations (nbl_read_state picks the c2v buffer per codeword)
	// layered (check-serial) schedule (nbl_create_layered / nbl_create_layered_ex / nbl_create_layered_bp): one c2v buffer updated in
	// place; EMS keeps no v2c, T-EMS (NBL_LAYERED_DAMPED) and log-QSPA keep the per-edge v2c their damping reads, updated in place by the
	// edge's check
	bool layered = false;
	bool fht = false;         // nbl_create_fht: the FHT sum-product check node in place of the exact one (flooding or layered)
	int n_layers = 0;
	std::vector<int> h_layer_of; // [M] the assignment in use
	std::vector<int> h_lay_off;  // [n_layers + 1] offsets into ly.chk
	NblLayerDev ly{};
	// device-side demodulator (nbl_set_demodulator)
	int dm_order = 0, dm_L = 0;
	double *d_cons = nullptr;
	int *d_src = nullptr;
	bool dm_general = false;           // the general kernel (nbl_demod.hip): d_dmdesc in place of d_src
	int dm_metric = 0;                 // NBL_DEMOD_*
	NblDemodPoint *d_dmdesc = nullptr; // [N][p + 1]
	double *d_rx = nullptr;
	size_t d_rx_cap = 0;
	// iterative demapping (nbl_decode_batch_samples_prior / _idd)
	int *d_tinv = nullptr;             // [L m] general path: the code bit that claims label bit t (the inverse of src), -1 = nobody
	double *d_prior = nullptr;         // staging of a host prior [B][N p]
	size_t d_prior_cap = 0;
	struct Idd {                       // buffers of the loop, grown on demand, counted in soft_bytes
		double *rx[2] = {nullptr, nullptr};  // samples of the survivors, ping-pong (pass k reads one, the gather fills the other)
		double *gain[2] = {nullptr, nullptr}; // their channel gains, when the call has gains
		size_t gain_cap[2] = {0, 0};
		int *idx[2] = {nullptr, nullptr};    // their batch positions
		double *ext = nullptr, *prior = nullptr; // extrinsic bit LLRs of a pass [n][N p]; the survivors' rows of it = the next prior
		int *res_out = nullptr, *res_iters = nullptr, *res_pass = nullptr; // [B][N], [B], [B]: results at batch positions
		uint8_t *res_done = nullptr;
		size_t rx_cap[2] = {0, 0}, idx_cap[2] = {0, 0}, ext_cap = 0, prior_cap = 0, out_cap = 0, iters_cap = 0, pass_cap = 0, done_cap = 0;
	} idd;
	// flat fading (nbl_set_fading, nbl_decode_batch_samples_csi)
	int fade_model = NBL_FADING_NONE, fade_coh = 1;
	uint32_t *d_jump_f = nullptr;      // [3][nblk + L] A^(4 k) mod m: the fading frame's positions (gains, then noise)
	int jump_f_pos = 0;                // the position count d_jump_f was made for
	double *d_gain = nullptr;          // [B][L][2] gains beside d_rx: staging of a host array, or what the channel of nbl_decode_batch_noise formed
	size_t d_gain_cap = 0;
	bool rx_gain = false;              // d_gain holds the gains of the samples in d_rx
	double *d_gains[2] = {nullptr, nullptr}; // resident gains beside d_rxs, one per slot (filled on the channel thread)
	size_t d_gains_cap[2] = {0, 0};
	bool slot_gain[2] = {false, false};      // the slot's samples were formed under fading: its gains are valid
	bool idd_sub = false;              // the last decode call was a loop with passes > 1: the workspace holds its last sub-batch
	// bit-LLR input and soft output (nbl_decode_batch_bits, nbl_soft_output): staging of the host forms, grown on demand
	double *d_lam = nullptr, *d_soft_sym = nullptr, *d_soft_bit = nullptr;
	size_t d_lam_cap = 0, d_soft_sym_cap = 0, d_soft_bit_cap = 0;
	size_t soft_bytes = 0;      // their sum: part of nbl_workspace_bytes from the moment they exist
	// device-side AWGN channel (nbl_decode_batch_noise)
	std::vector<double> h_cons;  // constellation as given to nbl_set_demodulator
	uint32_t *d_jump = nullptr;  // [3][L] A^(4 s) mod m of the three generators
	uint32_t *d_state = nullptr; // [cap][3]
	uint8_t *d_txi = nullptr;    // [cap][L]
	double *d_fn = nullptr;      // [cap][L][2][2]: log(1 - u1), cos(2 pi u2) of every normal draw
	uint32_t *d_fidx = nullptr;  // uncertain values: index into d_fn, argument, host-evaluated value
	double *d_farg = nullptr, *d_fval = nullptr;
	unsigned *d_fcount = nullptr;
	uint32_t *h_fidx = nullptr;  // pinned host mirrors
	double *h_farg = nullptr, *h_fval = nullptr;
	size_t noise_cap = 0, noise_pos = 0, flag_cap = 0;
	double last_flag_frac = 0.0;
	hipStream_t stream2 = nullptr; // the channel of batch k+1 runs here while batch k is decoded on `stream`
	double *d_rxs[2] = {nullptr, nullptr}; // resident received samples of nbl_channel_batch, one per slot
	size_t d_rxs_cap[2] = {0, 0};
	int rxs_B[2] = {0, 0};
	// device-side transmitter and error count (nbl_set_transmitter)
	struct Tx {
		bool on = false;
		int crc_len = 0, random_msg = 0, K = 0, nb = 0, nw = 0, nwg = 0, mb = 0, period = 1, par_mod = 0;
		unsigned long long *T = nullptr, *G = nullptr; // [nw][N p] PN bits -> code bits; [nwg][N p] message bits -> code bits (= T when crc_len == 0)
		int *keep = nullptr;          // [L mb] code bit carried by every modulator bit
		uint32_t *crc_col = nullptr;  // [K p] remainder of message bit i under CrcCheck's type-1 polynomial
		int16_t *phase_of = nullptr;  // [2048] register state -> position in seq, -1 = all-zero output
		uint8_t *seq = nullptr;       // [period] output bit of the register along its cycle
		uint16_t *pn = nullptr;       // [cap] staging of pn_state
		unsigned long long *u = nullptr; // [cap][nw]
		uint8_t *bits = nullptr;      // [cap][N p]
		size_t cap = 0;
		uint8_t *code[2] = {nullptr, nullptr}, *txi[2] = {nullptr, nullptr}; // per slot: [B][N] code symbols, [B][L] constellation indices
		size_t slot_cap[2] = {0, 0};
		int tx_B[2] = {0, 0};
		int *dec[2] = {nullptr, nullptr}; // per slot: outputs of the last nbl_decode_batch_resident
		size_t dec_cap[2] = {0, 0};
		int dec_B[2] = {0, 0};
		int *cnt = nullptr;           // [cnt_cap] err_sym, [cnt_cap] err_bit, then [cnt_cap] bytes crc_ok
		size_t cnt_cap = 0;
		// nbl_encode_batch scratch (decode thread)
		int *e_msg = nullptr; unsigned long long *e_u = nullptr; uint8_t *e_bits = nullptr, *e_code = nullptr;
		size_t e_cap = 0;
	} tx;
	std::string err2;              // error text of the channel thread (nbl_channel_batch); nbl_last_error reports both
	// hipGraph replay of the iteration loop: one executable graph per window of iterations (fixed iterations: the whole loop;
	// early exit: the `poll_every` iterations between two polls), captured on the decoder's own stream the first time a window is
	// run with a given set of buffers, replayed on the caller's stream afterwards.  NBL_GRAPH=0 switches it off.
	struct GraphKey { const void *lin, *lch, *v2c, *c2v, *alt, *post, *osd_s; int B, record, generic, fused; };
	GraphKey gkey{};
	std::vector<hipGraphExec_t> gexec; // index = window number
	int *d_active = nullptr;           // [cap] active list (early exit, batches of NBL_COMPACT_MIN codewords or more)
	bool use_compact = true;           // NBL_COMPACT=0 switches it off
	bool use_graph = false;            // opt-in (NBL_GRAPH=1): measured gain is nil, see DESIGN.md section 7
	int force_generic = 0;      // debug: 1 = always the generic kernels, 2 = specialised kernels but no VN/CN fusion
	bool profiling = false;
	hipEvent_t ev[2] = {nullptr, nullptr};
	int *h_ndone = nullptr;      // pinned [2]: converged-codeword counts read back after each window of iterations
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

static int ilog2(int q)
{
	int p = 0;
	while ((1 << p) < q) p++;
	return p;
}

template <typename T> static nbl_status upload(nbl_decoder *d, const std::vector<T> &h, const T **dst)
{
	void *p = nullptr;
	HIP_TRY(d, hipMalloc(&p, h.size() * sizeof(T) + 16));
	d->graph_allocs.push_back(p);
	HIP_TRY(d, hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
	*dst = (const T *)p;
	return NBL_OK;
}

static void drop_graphs(nbl_decoder *d)
{
	for (auto &ge : d->gexec)
		if (ge) (void)hipGraphExecDestroy(ge);
	d->gexec.clear();
}

static void free_workspace(nbl_decoder *d)
{
	drop_graphs(d);
	void *ptrs[] = {d->w.Lch, d->w.v2c, d->w.c2v, d->w.post, d->w.dec, d->w.out, d->w.iters, d->w.done, d->d_Lin, d->d_conv8, d->c2v_alt, d->w.edge_dec, d->d_active, d->c2v_zero, d->osd_S};
	d->osd_S = nullptr;
	d->c2v_zero = nullptr;
	d->d_active = nullptr;
	d->w.active = nullptr;
	d->c2v_alt = nullptr;
	for (void *p : ptrs)
		if (p) (void)hipFree(p);
	d->w.Lch = d->w.v2c = d->w.c2v = d->w.post = nullptr;
	d->w.dec = d->w.out = d->w.iters = d->w.edge_dec = nullptr;
	d->w.done = nullptr;
	d->d_Lin = nullptr;
	d->d_conv8 = nullptr;
	d->cap = 0;
	d->ws_bytes = 0;
	d->last_B = 0; // (nothing of the last decode call is left to read)
	d->last_c2v = nullptr;
}

static bool small_enabled()
{
	static const bool on = !getenv("NBL_NO_SMALL"); // A/B measurements: the several-checks-per-wave kernels on small fields
	return on;
}

// The kernel choice of this decoder as it stands (nbl_plan.cpp): once per workspace check and once per decode, never per launch
static NblPlan plan_of(const nbl_decoder *d)
{
	return nbl_plan(d->shape, d->prm, d->ext, d->layered, d->force_generic, d->record_state, small_enabled(), d->fht);
}

static nbl_status ensure_workspace(nbl_decoder *d, int B)
{
	const NblPlan plan = plan_of(d);
	const bool want_v2c = plan.want_v2c;
	const bool want_post = d->record_state || d->osd_acc;
	if (B <= d->cap && (!want_post || d->w.post) && (!want_v2c || d->w.v2c)) return NBL_OK;
	int cap = B > d->cap ? B : d->cap;
	free_workspace(d);
	const size_t q = d->g.q, N = d->g.N, E = d->g.E;
	size_t bytes = 0;
	auto alloc = [&](void **p, size_t n) -> hipError_t { bytes += n; return hipMalloc(p, n); };
	HIP_TRY(d, alloc((void **)&d->w.Lch, (size_t)cap * N * q * 8));
	if (want_v2c) HIP_TRY(d, alloc((void **)&d->w.v2c, (size_t)cap * E * q * 8));
	HIP_TRY(d, alloc((void **)&d->w.c2v, (size_t)cap * E * q * 8));
	if (plan.fusable) { // (whatever force_generic says: nbl_workspace_bytes does not move with a debug switch)
		HIP_TRY(d, alloc((void **)&d->c2v_alt, (size_t)cap * E * q * 8));
		HIP_TRY(d, alloc((void **)&d->c2v_zero, E * q * 8)); // one block for every codeword (NblWork::c2v_prev_shared)
		HIP_TRY(d, hipMemset(d->c2v_zero, 0, E * q * 8));
	}
	if (want_post) HIP_TRY(d, alloc((void **)&d->w.post, (size_t)cap * N * q * 8));
	if (d->osd_acc) HIP_TRY(d, alloc((void **)&d->osd_S, (size_t)cap * N * d->g.p * 8));
	HIP_TRY(d, alloc((void **)&d->w.dec, (size_t)cap * N * 4));
	if (d->prm.method != NBL_METHOD_EMS) HIP_TRY(d, alloc((void **)&d->w.edge_dec, (size_t)cap * E * 4));
	HIP_TRY(d, alloc((void **)&d->w.out, (size_t)cap * N * 4));
	HIP_TRY(d, alloc((void **)&d->w.iters, (size_t)cap * 4));
	HIP_TRY(d, alloc((void **)&d->w.done, (size_t)cap));
	HIP_TRY(d, alloc((void **)&d->d_active, (size_t)cap * 4));
	d->cap = cap;
	d->ws_bytes = bytes;
	return NBL_OK;
}

extern "C" int32_t nbl_abi_version(void) { return NBL_ABI_VERSION; }

extern "C" const char *nbl_last_error(const nbl_decoder *dec)
{
	if (!dec) return g_create_error.c_str();
	if (dec->err2.empty()) return dec->err.c_str();
	if (dec->err.empty()) return dec->err2.c_str();
	static thread_local std::string both;
	both = dec->err + " | channel: " + dec->err2;
	return both.c_str();
}

extern "C" size_t nbl_workspace_bytes(const nbl_decoder *dec)
{
	return dec ? dec->ws_bytes + dec->soft_bytes + dec->d_gain_cap + dec->d_gains_cap[0] + dec->d_gains_cap[1] : 0;
}

static nbl_status fail_create(nbl_decoder *d, nbl_status st, const std::string &msg)
{
	g_create_error = msg.empty() && d ? d->err : msg;
	if (d) nbl_destroy(d);
	return st;
}

extern "C" nbl_status nbl_create(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                                 const nbl_params *params, int device, nbl_decoder **out)
{
	return nbl_create_ex(code, gf_mul, gf_inv, params, nullptr, device, out);
}

extern "C" nbl_status nbl_create_ex(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                                    const nbl_params *params, const nbl_params_ext *ext, int device, nbl_decoder **out)
{
	return nbl_create_osd(code, gf_mul, gf_inv, params, ext, nullptr, device, out);
}

// G_GaussEliminate_bit (OSD.h:258-324), literally: forward elimination with the pivot repair from the rows below and the rotation of
// order[row..] when no row has the bit
static void g_gauss_eliminate(std::vector<std::vector<uint8_t>> &m, int col_length, int row_length, std::vector<int> &order)
{
	for (int row = 0; row < row_length; row++) {
		int col = order[row];
		if (m[row][col] == 0) {
			bool exchanged = false;
			for (int up = row + 1; up < row_length; up++)
				if (m[up][col] != 0) {
					for (int i = 0; i < col_length; i++) m[row][i] ^= m[up][i];
					exchanged = true;
					break;
				}
			if (!exchanged) {
				const int flag = row;
				row--;
				for (int i = flag; i < col_length - 1; i++) std::swap(order[i], order[i + 1]);
			}
		}
		for (int up = row + 1; up < row_length; up++)
			if (m[up][col] != 0)
				for (int i = 0; i < col_length; i++) m[up][i] ^= m[row][i];
	}
	for (int row = row_length - 1; row > 0; row--)
		for (int up = row - 1; up >= 0; up--)
			if (m[up][order[row]] == 1)
				for (int i = 0; i < col_length; i++) m[up][i] ^= m[row][i];
}

// [CRC rows; H_bit] of Decoding_OSD_bit (OSD.h:44-57): H_bit as CNBLDPC::Initial builds it (NBLDPC.cpp:416-430, plain assignment in
// variable-major edge order), the CRC rows as CRCMatrixGen (OSD.h:472-509).  Returns the rows, or an error text.
static std::string osd_matrix(const nbl_code_desc *code, int p, const nbl_osd_params *o, std::vector<std::vector<uint8_t>> &rows)
{
	const int N = code->N, M = code->M, n = N * p, Mb = M * p, msg = n - Mb, L = o->crc_len, cr = o->crc_rows;
	std::vector<std::vector<uint8_t>> H((size_t)Mb, std::vector<uint8_t>(n, 0));
	for (int v = 0, e = 0; v < N; v++)
		for (int j = 0; j < code->var_deg[v]; j++, e++) {
			const int chk = code->var_chk[e], h = code->var_h[e];
			for (int k = 0; k < p; k++)
				for (int l = 0; l < p; l++) H[(size_t)p * chk + k][(size_t)p * v + l] = o->gf_mat[((size_t)h * p + l) * p + k];
		}
	rows.clear();
	if (cr > 0) {
		if (msg - L <= 0) return "OSD: the CRC generator has no rows (crc_len >= N p - M p)";
		std::vector<std::vector<uint8_t>> G((size_t)(msg - L), std::vector<uint8_t>(msg, 0));
		static const int taps8[] = {0, 1, 4, 5, 7, 8}, taps16[] = {0, 4, 11, 16}, taps24[] = {0, 1, 18, 19, 23, 24};
		const int *taps = L == 8 ? taps8 : L == 16 ? taps16 : taps24;
		const int ntaps = L == 16 ? 4 : 6;
		for (int i = 0; i < msg - L; i++)
			for (int t = 0; t < ntaps; t++) G[i][i + taps[t]] = 1;
		std::vector<int> seri(msg);
		for (int i = 0; i < msg; i++) seri[i] = i;
		g_gauss_eliminate(G, msg, msg - L, seri);
		for (int i = 0; i < cr; i++) {
			std::vector<uint8_t> r(n, 0);
			r[i + msg - cr] = 1;
			for (int j = 0; j < msg - L; j++) r[j] = G[j][msg - cr + i];
			rows.push_back(r);
		}
	}
	for (auto &r : H) rows.push_back(r);
	return "";
}

// GF(2) rank of a row set (column order does not matter)
static int gf2_rank(std::vector<std::vector<uint64_t>> m, int nw)
{
	int rank = 0;
	const int R = (int)m.size();
	for (int c = 0; c < nw * 64 && rank < R; c++) {
		int piv = -1;
		for (int r = rank; r < R; r++)
			if ((m[r][c >> 6] >> (c & 63)) & 1) { piv = r; break; }
		if (piv < 0) continue;
		std::swap(m[piv], m[rank]);
		for (int r = 0; r < R; r++)
			if (r != rank && ((m[r][c >> 6] >> (c & 63)) & 1))
				for (int x = 0; x < nw; x++) m[r][x] ^= m[rank][x];
		rank++;
	}
	return rank;
}

// The caller's field tables, checked in full before anything is indexed by one of their entries: gf_mul must be THE table of
// GF(2)[x] / poly in the polynomial basis (poly read off x * x^(p-1)), gf_inv its inverses.  Some kernels multiply by shift and
// XOR with poly, others look gf_mul up as bytes or through offsets built from it: they decode the same code only if the whole
// table is that product.  Every non-zero element has an inverse exactly when poly is irreducible, so a reducible modulus is
// refused by the last condition.  Returns poly, or 0 with the first offending entry named in `msg`.
static int validate_field(int q, const uint16_t *gf_mul, const uint16_t *gf_inv, std::string &msg)
{
	const int p = ilog2(q);
	for (int a = 0; a < q; a++)
		for (int b = 0; b < q; b++)
			if (gf_mul[(size_t)a * q + b] >= q) {
				msg = "gf_mul[" + std::to_string(a) + "][" + std::to_string(b) + "] = " + std::to_string(gf_mul[(size_t)a * q + b]) + " is not an element of GF(" + std::to_string(q) + ")";
				return 0;
			}
	for (int a = 0; a < q; a++)
		if (gf_mul[a] != 0 || gf_mul[(size_t)a * q] != 0) {
			const bool row = gf_mul[a] != 0;
			msg = "gf_mul[" + std::to_string(row ? 0 : a) + "][" + std::to_string(row ? a : 0) + "] is not zero";
			return 0;
		}
	// x * x^(p-1) = x^p = poly - q
	const int poly = q | gf_mul[(size_t)2 * q + (q >> 1)];
	for (int a = 1; a < q; a++)
		for (int b = 1; b < q; b++) {
			int acc = 0, x = a;
			for (int i = 0; i < p; i++) {
				if ((b >> i) & 1) acc ^= x;
				x <<= 1;
				if (x & q) x ^= poly;
			}
			if (gf_mul[(size_t)a * q + b] != acc) {
				msg = "gf_mul is not a polynomial-basis GF(2^p) table: gf_mul[" + std::to_string(a) + "][" + std::to_string(b) + "] = " + std::to_string(gf_mul[(size_t)a * q + b]) +
				      ", the product modulo " + std::to_string(poly) + " is " + std::to_string(acc);
				return 0;
			}
		}
	for (int a = 1; a < q; a++) {
		if (gf_inv[a] >= q) {
			msg = "gf_inv[" + std::to_string(a) + "] = " + std::to_string(gf_inv[a]) + " is not an element of GF(" + std::to_string(q) + ")";
			return 0;
		}
		if (gf_mul[(size_t)a * q + gf_inv[a]] != 1) {
			msg = "gf_inv inconsistent with gf_mul: gf_mul[" + std::to_string(a) + "][gf_inv[" + std::to_string(a) + "] = " + std::to_string(gf_inv[a]) + "] is not 1 (modulus " +
			      std::to_string(poly) + "; a reducible modulus has elements without an inverse)";
			return 0;
		}
	}
	return poly;
}

// ---- layer assignments of the layered schedule (include/nbldpc.h): pure host arithmetic --------------------------------------
// Greedy colouring on a checked graph: checks in ascending index, each gets the smallest layer that holds no check sharing a
// variable with it.  Returns the number of layers.
static int layer_greedy(int N, int M, const std::vector<int> &coff, const int32_t *chk_var, int32_t *layer_of)
{
	std::vector<std::vector<int>> used(N);  // layers of the checks each variable has joined so far
	std::vector<int> stamp(M + 1, -1);
	int n_layers = 0;
	for (int m = 0; m < M; m++) {
		for (int ce = coff[m]; ce < coff[m + 1]; ce++)
			for (int l : used[chk_var[ce]]) stamp[l] = m;
		int l = 0;
		while (stamp[l] == m) l++; // (at most M - 1 layers are taken: stamp[M] is never reached)
		layer_of[m] = l;
		if (l + 1 > n_layers) n_layers = l + 1;
		for (int ce = coff[m]; ce < coff[m + 1]; ce++) {
			std::vector<int> &u = used[chk_var[ce]];
			bool have = false;
			for (int x : u) have = have || x == l;
			if (!have) u.push_back(l);
		}
	}
	return n_layers;
}

// A caller's assignment: every index >= 0, every layer up to the largest index used non-empty, no two checks of a layer sharing a
// variable.  Returns the number of layers, or 0 with the offence named in `msg`.
static int layer_validate(int N, int M, const std::vector<int> &coff, const int32_t *chk_var, const int32_t *layer_of, std::string &msg)
{
	int n_layers = 0;
	for (int m = 0; m < M; m++) {
		if (layer_of[m] < 0) { msg = "layered schedule: layer_of[" + std::to_string(m) + "] = " + std::to_string(layer_of[m]) + " is below 0"; return 0; }
		if (layer_of[m] >= M) { msg = "layered schedule: layer " + std::to_string(layer_of[m]) + " of check " + std::to_string(m) + " leaves an empty layer below it (M = " + std::to_string(M) + " checks)"; return 0; }
		if (layer_of[m] + 1 > n_layers) n_layers = layer_of[m] + 1;
	}
	std::vector<int> count(n_layers, 0);
	for (int m = 0; m < M; m++) count[layer_of[m]]++;
	for (int l = 0; l < n_layers; l++)
		if (!count[l]) { msg = "layered schedule: layer " + std::to_string(l) + " is empty (the largest layer index used is " + std::to_string(n_layers - 1) + ")"; return 0; }
	// per variable: the check that claimed each layer first
	std::vector<std::vector<std::pair<int, int>>> seen(N);
	for (int m = 0; m < M; m++)
		for (int ce = coff[m]; ce < coff[m + 1]; ce++) {
			const int n = chk_var[ce];
			for (const auto &pr : seen[n])
				if (pr.first == layer_of[m] && pr.second != m) {
					msg = "layered schedule: checks " + std::to_string(pr.second) + " and " + std::to_string(m) + " of layer " + std::to_string(layer_of[m]) + " share variable " + std::to_string(n);
					return 0;
				}
			seen[n].push_back({layer_of[m], m});
		}
	return n_layers;
}

extern "C" int32_t nbl_layer_greedy(const nbl_code_desc *code, int32_t *layer_of)
{
	if (!code || !layer_of || !code->chk_deg || !code->chk_var) { g_create_error = "null argument"; return NBL_ERR_ARG; }
	const int N = code->N, M = code->M;
	if (N <= 0 || M <= 0) { g_create_error = "N, M must be positive"; return NBL_ERR_ARG; }
	std::vector<int> coff(M + 1, 0);
	for (int m = 0; m < M; m++) {
		if (code->chk_deg[m] < 1 || code->chk_deg[m] > N) { g_create_error = "check degree out of range"; return NBL_ERR_ARG; }
		coff[m + 1] = coff[m] + code->chk_deg[m];
	}
	for (int ce = 0; ce < coff[M]; ce++)
		if (code->chk_var[ce] < 0 || code->chk_var[ce] >= N) { g_create_error = "check-side edge out of range"; return NBL_ERR_ARG; }
	return layer_greedy(N, M, coff, code->chk_var, layer_of);
}

// nbl_create_layered's / nbl_create_layered_ex's / nbl_create_layered_bp's request: layer_of == NULL asks for the greedy assignment;
// flags: NBL_LAYERED_*; bp: the log-QSPA entry point (method 1 alone, its own damping: no flag)
struct LayerReq { const int32_t *layer_of; uint32_t flags; bool bp; };

static nbl_status create_impl(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                              const nbl_params_ext *ext, const nbl_osd_params *osd, const LayerReq *lay, int device, nbl_decoder **out,
                              bool fht = false);

extern "C" nbl_status nbl_create_osd(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                     const nbl_params_ext *ext, const nbl_osd_params *osd, int device, nbl_decoder **out)
{
	return create_impl(code, gf_mul, gf_inv, params, ext, osd, nullptr, device, out);
}

extern "C" nbl_status nbl_create_layered(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                         const int32_t *layer_of, int device, nbl_decoder **out)
{
	const LayerReq lay = {layer_of, 0, false};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, &lay, device, out);
}

extern "C" nbl_status nbl_create_layered_ex(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                            const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	const LayerReq lay = {layer_of, flags, false};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, &lay, device, out);
}

extern "C" nbl_status nbl_create_layered_bp(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                            const int32_t *layer_of, int device, nbl_decoder **out)
{
	const LayerReq lay = {layer_of, 0, true};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, &lay, device, out);
}

// FHT sum-product decoding (include/nbldpc.h): flooding without a LayerReq, layered with the request of nbl_create_layered_bp -- the same
// assignment rules, the same v2c state
extern "C" nbl_status nbl_create_fht(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                     const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	if (!out) return NBL_ERR_ARG;
	*out = nullptr;
	if (flags & ~(uint32_t)NBL_FHT_LAYERED)
		return fail_create(nullptr, NBL_ERR_ARG, "nbl_create_fht: unknown flag bit (flags = " + std::to_string(flags) + "; NBL_FHT_LAYERED = 1 is the only one defined)");
	if (!(flags & NBL_FHT_LAYERED) && layer_of)
		return fail_create(nullptr, NBL_ERR_ARG, "nbl_create_fht: a layer assignment belongs to the layered schedule (flags = 0 is flooding: pass layer_of = NULL, or set "
		                                         "NBL_FHT_LAYERED)");
	const LayerReq lay = {layer_of, 0, true};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, (flags & NBL_FHT_LAYERED) ? &lay : nullptr, device, out, true);
}

extern "C" nbl_status nbl_get_layers(const nbl_decoder *d, int32_t *layer_of, int32_t *n_layers)
{
	if (!d || !d->layered) return NBL_ERR_ARG;
	if (layer_of) memcpy(layer_of, d->h_layer_of.data(), d->h_layer_of.size() * sizeof(int32_t));
	if (n_layers) *n_layers = d->n_layers;
	return NBL_OK;
}

static nbl_status create_impl(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                              const nbl_params_ext *ext, const nbl_osd_params *osd, const LayerReq *lay, int device, nbl_decoder **out, bool fht)
{
	if (!out) return NBL_ERR_ARG;
	*out = nullptr;
	if (!code || !gf_mul || !gf_inv || !params) return fail_create(nullptr, NBL_ERR_ARG, "null argument");
	if (lay && (lay->flags & ~(uint32_t)NBL_LAYERED_DAMPED))
		return fail_create(nullptr, NBL_ERR_ARG, "layered schedule: unknown flag bit (flags = " + std::to_string(lay->flags) + "; NBL_LAYERED_DAMPED = 1 is the only one defined)");
	const int N = code->N, M = code->M, q = code->q;
	if (N <= 0 || M <= 0 || q < 4 || (q & (q - 1))) return fail_create(nullptr, NBL_ERR_ARG, "N, M must be positive and q a power of two, at least 4");
	// (the reference ships arithmetic tables up to GF(512) but no code above GF(256); a valid request this library cannot serve)
	if (q > 256) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "fields above GF(256) are not supported (one wave holds at most 4 symbols per lane)");
	std::string field_err;
	const int poly = validate_field(q, gf_mul, gf_inv, field_err);
	if (!poly) return fail_create(nullptr, NBL_ERR_ARG, field_err);
	if (fht && params->method != NBL_METHOD_BP)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "nbl_create_fht runs the sum-product rule of log-QSPA (method 1) only: the transform evaluates its XOR convolution, "
		                                                 "which no other method's check node is");
	if (lay && lay->bp && params->method != NBL_METHOD_BP)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "nbl_create_layered_bp runs log-QSPA (method 1) only: the layered schedule of EMS (method 2) is behind "
		                                                 "nbl_create_layered, that of T-EMS (method 4) behind nbl_create_layered_ex with NBL_LAYERED_DAMPED");
	if (lay && !lay->bp && (lay->flags & NBL_LAYERED_DAMPED) && params->method != NBL_METHOD_EMS && params->method != NBL_METHOD_TEMS)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "the damped layered schedule (NBL_LAYERED_DAMPED) is defined for T-EMS (method 4), and for EMS (method 2), which "
		                                                 "has no damping, as the plain layered schedule: log-QSPA (method 1) and BS-TEMS (method 7) stay flooding-only");
	if (lay && !lay->bp && params->method != NBL_METHOD_EMS && !((lay->flags & NBL_LAYERED_DAMPED) && params->method == NBL_METHOD_TEMS))
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "the layered schedule is defined for EMS (method 2) only: the other methods damp against the previous iteration's "
		                                                 "decision in their variable-node pass and stay flooding-only");
	switch (params->method) {
	case NBL_METHOD_EMS: case NBL_METHOD_BP: case NBL_METHOD_TEMS: break;
	case NBL_METHOD_BS_TEMS:
		if (!ext) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "BS-TEMS (method 7): its parameters (bs_nm, bs_nc, bs_factor, bs_offset) go through nbl_create_ex");
		break;
	case NBL_METHOD_OSD:
		if (!osd) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD (method 6): its parameters (order, flag, factor, crc_len, crc_rows, gf_mat) go through nbl_create_osd");
		break;
	default: return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "decode method not supported (reference: 'has not been developed')");
	}
	// ---- OSD parameters and the binary matrix, before any device call ----
	const bool osd_on = osd && (params->method == NBL_METHOD_OSD || osd->order >= 0);
	std::vector<uint64_t> osd_words;
	int osd_R = 0;
	if (osd) {
		if (osd->order < -1) return fail_create(nullptr, NBL_ERR_ARG, "OSD: order < -1");
		if (osd->flag != 0 && osd->flag != 1) return fail_create(nullptr, NBL_ERR_ARG, "OSD: flag must be 0 or 1");
		if (!osd->gf_mat) return fail_create(nullptr, NBL_ERR_ARG, "OSD: gf_mat is NULL");
		for (int p1 = ilog2(q), i = 0; i < p1 * p1; i++) // the matrix of "multiply by 1"
			if (osd->gf_mat[(size_t)p1 * p1 + i] != (i / p1 == i % p1))
				return fail_create(nullptr, NBL_ERR_ARG, "OSD: gf_mat of element 1 is not the identity (entry [" + std::to_string(i / p1) + "][" + std::to_string(i % p1) + "])");
		if (osd->crc_rows < 0 || osd->crc_rows > osd->crc_len) return fail_create(nullptr, NBL_ERR_ARG, "OSD: crc_rows must be in 0 .. crc_len");
		if (osd->crc_rows > 0 && osd->crc_len != 8 && osd->crc_len != 16 && osd->crc_len != 24)
			return fail_create(nullptr, NBL_ERR_ARG, "OSD: CRC rows need crc_len 8, 16 or 24 (the reference's CRC generator is empty otherwise and its elimination never ends)");
	}
	if (osd_on) {
		const int p = ilog2(q), n = N * p;
		// (every n up to the cap fits: nbl_osd_lds_bytes(1024, .) = 160,464 B of the 163,840 B of one workgroup; checked here, before any
		// device call, so that a change of either limit cannot reach the first decode)
		if (n > NBL_OSD_MAX_BITS || nbl_osd_lds_bytes(n, 0) > NBL_OSD_MAX_LDS)
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD: N log2(q) above NBL_OSD_MAX_BITS (1024) does not fit the kernel's LDS");
		for (int v = 0, e = 0; v < N; v++) // (the graph is validated below; the matrix build must not index outside it first)
			for (int j = 0; j < code->var_deg[v]; j++, e++)
				if (code->var_deg[v] < 1 || code->var_chk[e] < 0 || code->var_chk[e] >= M || code->var_h[e] <= 0 || code->var_h[e] >= q)
					return fail_create(nullptr, NBL_ERR_ARG, "variable-side edge out of range");
		std::vector<std::vector<uint8_t>> rows;
		const std::string e = osd_matrix(code, p, osd, rows);
		if (!e.empty()) return fail_create(nullptr, NBL_ERR_ARG, e);
		osd_R = (int)rows.size();
		if (osd_R >= n) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD: the matrix has no fewer rows than columns");
		const int nw = (n + 63) / 64;
		std::vector<std::vector<uint64_t>> packed(osd_R, std::vector<uint64_t>(nw, 0));
		for (int r = 0; r < osd_R; r++)
			for (int c = 0; c < n; c++)
				if (rows[r][c]) packed[r][c >> 6] |= 1ull << (c & 63);
		if (gf2_rank(packed, nw) != osd_R)
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD: [CRC rows; H_bit] is not of full row rank (the reference's elimination never ends on it)");
		for (auto &r : packed) osd_words.insert(osd_words.end(), r.begin(), r.end());
	}
	if (params->max_iter < 0) return fail_create(nullptr, NBL_ERR_ARG, "max_iter < 0");
	if (params->method == NBL_METHOD_EMS) {
		// reference: "EMS configuration error! EMS_Nm is too large!" + exit(-1), NBLDPC.cpp:282-286
		if (params->ems_nm > q) return fail_create(nullptr, NBL_ERR_ARG, "EMS configuration error! EMS_Nm is too large!");
		if (params->ems_nm < 1 || params->ems_nc < 0) return fail_create(nullptr, NBL_ERR_ARG, "ems_nm < 1 or ems_nc < 0");
	}
	if (params->method == NBL_METHOD_TEMS && (params->tems_nr < 1 || params->tems_nc < 0))
		return fail_create(nullptr, NBL_ERR_ARG, "tems_nr < 1 or tems_nc < 0");
	if (params->method == NBL_METHOD_BS_TEMS) {
		// the reference's basic-set arrays hold q elements (NBLDPC.cpp:333): bs_nm >= q reads past them
		if (ext->bs_nm < 1 || ext->bs_nm >= q) return fail_create(nullptr, NBL_ERR_ARG, "BS-TEMS: bs_nm must be at least 1 and below q");
		if (ext->bs_nc < 0) return fail_create(nullptr, NBL_ERR_ARG, "BS-TEMS: bs_nc < 0");
		if (!(ext->bs_factor != 0.0)) return fail_create(nullptr, NBL_ERR_ARG, "BS-TEMS: bs_factor must be non-zero (c2v values are divided by it)");
		if (ext->bs_nm > 16)
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "BS-TEMS: bs_nm above 16 is not supported (the kernel enumerates configurations as bs_nm-bit masks)");
	}

	// ---- host-side graph indices (NBLDPC.cpp:236-263) -------------------------------------------------------
	std::vector<int> voff(N + 1, 0), coff(M + 1, 0);
	const NblShape shape = nbl_shape(code);
	const int maxdv = shape.maxdv, maxdc = shape.maxdc, p = shape.p;
	for (int n = 0; n < N; n++) {
		if (code->var_deg[n] < 1) return fail_create(nullptr, NBL_ERR_ARG, "variable of degree < 1");
		voff[n + 1] = voff[n] + code->var_deg[n];
	}
	for (int m = 0; m < M; m++) {
		if (code->chk_deg[m] < 2) return fail_create(nullptr, NBL_ERR_ARG, "check of degree < 2");
		coff[m + 1] = coff[m] + code->chk_deg[m];
	}
	const int E = voff[N];
	if (coff[M] != E) return fail_create(nullptr, NBL_ERR_ARG, "variable-side and check-side edge counts differ");
	if (maxdc > NBL_MAXDC || maxdv > NBL_MAXDV) return fail_create(nullptr, NBL_ERR_ARG, "node degree above the supported maximum (8)");
	std::vector<int> v_cpos(E, -1), c_epos(E, -1), c_var(E), c_h(E), c_hinv(E);
	for (int ce = 0; ce < E; ce++) {
		int n = code->chk_var[ce], h = code->chk_h[ce];
		if (n < 0 || n >= N || h <= 0 || h >= q) return fail_create(nullptr, NBL_ERR_ARG, "check-side edge out of range / zero coefficient");
		c_var[ce] = n;
		c_h[ce] = h;
		c_hinv[ce] = gf_inv[h];
	}
	for (int n = 0; n < N; n++)
		for (int e = voff[n]; e < voff[n + 1]; e++) {
			int m = code->var_chk[e];
			if (m < 0 || m >= M) return fail_create(nullptr, NBL_ERR_ARG, "variable-side edge out of range");
			for (int ce = coff[m]; ce < coff[m + 1]; ce++)
				if (c_var[ce] == n) v_cpos[e] = ce; // last match wins, like VarLinkDc
			if (v_cpos[e] < 0 || c_h[v_cpos[e]] != code->var_h[e]) return fail_create(nullptr, NBL_ERR_ARG, "variable-side and check-side edge lists disagree");
		}
	for (int m = 0; m < M; m++)
		for (int ce = coff[m]; ce < coff[m + 1]; ce++) {
			int n = c_var[ce];
			for (int e = voff[n]; e < voff[n + 1]; e++)
				if (code->var_chk[e] == m) c_epos[ce] = e; // like ChkLinkDv
			if (c_epos[ce] < 0) return fail_create(nullptr, NBL_ERR_ARG, "check-side edge without variable-side partner");
		}
	// shape limits of the kernels, refused here rather than at the first decode
	if (params->method == NBL_METHOD_TEMS && p * maxdc > 32)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "T-EMS: log2(q) * (largest check degree) must not exceed 32 (the trellis path code is one 32-bit word)");
	if (params->method == NBL_METHOD_EMS && nbl_ems_lds_bytes(q, maxdc, params->ems_nm, params->ems_nc) > 160 * 1024)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "EMS: this (q, check degree, nm, nc) needs more than the 160 KB of LDS one wave can have");
	// ---- layered schedule: the assignment, checked or made here, before the device is touched ----
	std::vector<int> layer_of, lay_off, lay_chk, lay_nbr;
	int n_layers = 0;
	if (lay) {
		// (the layered kernel is the general one: no specialised shape stands in for it, so the LDS bound holds for every shape)
		// (log-QSPA: (3 maxdc + 5) q 8 bytes, at most 59,392 B at q = 256 and degree 8 -- nothing to refuse)
		if (params->method == NBL_METHOD_TEMS) {
			if (nbl_tems_layered_lds_bytes(q, maxdc, params->tems_nc) > 160 * 1024)
				return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "T-EMS: this (q, check degree, nc) needs more than the 160 KB of LDS one wave can have");
		} else if (params->method == NBL_METHOD_EMS && nbl_ems_lds_bytes(q, maxdc, params->ems_nm, params->ems_nc) > 160 * 1024) {
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "EMS: this (q, check degree, nm, nc) needs more than the 160 KB of LDS one wave can have");
		}
		layer_of.assign(M, 0);
		if (lay->layer_of) {
			std::string lerr;
			n_layers = layer_validate(N, M, coff, code->chk_var, lay->layer_of, lerr);
			if (!n_layers) return fail_create(nullptr, NBL_ERR_ARG, lerr);
			layer_of.assign(lay->layer_of, lay->layer_of + M);
		} else {
			n_layers = layer_greedy(N, M, coff, code->chk_var, layer_of.data());
		}
		lay_off.assign(n_layers + 1, 0);
		for (int m = 0; m < M; m++) lay_off[layer_of[m] + 1]++;
		for (int l = 0; l < n_layers; l++) lay_off[l + 1] += lay_off[l];
		lay_chk.assign(M, 0);
		std::vector<int> fill(lay_off.begin(), lay_off.end() - 1);
		for (int m = 0; m < M; m++) lay_chk[fill[layer_of[m]]++] = m;
		lay_nbr.assign((size_t)E * NBL_LAYER_ROW, 0);
		for (int ce = 0; ce < E; ce++) {
			const int n = c_var[ce], e0 = voff[n], dv = voff[n + 1] - e0;
			lay_nbr[(size_t)ce * NBL_LAYER_ROW] = n;
			lay_nbr[(size_t)ce * NBL_LAYER_ROW + 1] = dv;
			for (int k = 0; k < dv; k++) lay_nbr[(size_t)ce * NBL_LAYER_ROW + 4 + k] = v_cpos[e0 + k];
		}
	}

	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail_create(nullptr, NBL_ERR_NO_DEVICE, "no HIP device (this library has no CPU decode path)");
	if (device < 0 || device >= ndev) return fail_create(nullptr, NBL_ERR_ARG, "device index out of range");

	nbl_decoder *d = new nbl_decoder();
	d->device = device;
	d->prm = *params;
	if (params->method == NBL_METHOD_BS_TEMS) d->ext = *ext;
	if (hipSetDevice(device) != hipSuccess) return fail_create(d, NBL_ERR_HIP, "hipSetDevice failed");
	if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return fail_create(d, NBL_ERR_HIP, "hipStreamCreate failed");
	if (const char *e = getenv("NBL_GRAPH")) d->use_graph = atoi(e) != 0;
	if (const char *e = getenv("NBL_COMPACT")) d->use_compact = atoi(e) != 0;
	d->g.N = N; d->g.M = M; d->g.E = E; d->g.q = q; d->g.p = p; d->g.poly = poly; d->g.maxdc = maxdc; d->g.maxdv = maxdv;
	std::vector<uint8_t> mul8((size_t)q * q);
	for (size_t i = 0; i < mul8.size(); i++) mul8[i] = (uint8_t)gf_mul[i];
	nbl_status st;
	if ((st = upload(d, voff, &d->g.voff)) || (st = upload(d, coff, &d->g.coff)) || (st = upload(d, v_cpos, &d->g.v_cpos)) ||
	    (st = upload(d, c_epos, &d->g.c_epos)) || (st = upload(d, c_var, &d->g.c_var)) || (st = upload(d, c_h, &d->g.c_h)) ||
	    (st = upload(d, c_hinv, &d->g.c_hinv)) || (st = upload(d, mul8, &d->g.mul)))
		return fail_create(d, st, "");
	if (osd_on) {
		if ((st = upload(d, osd_words, &d->osd.H))) return fail_create(d, st, "");
		d->osd_on = true;
		d->osd.R = osd_R;
		d->osd.n_dist = (int)(N * std::log((double)q) / std::log(2.0)); // compute_min_distance_bit's CodeLen_bit, truncated like it
		d->osd.order = osd->order < 0 ? 0 : osd->order; // (method 6 runs order 0 when the profile's order is -1)
		d->osd.flag = params->method == NBL_METHOD_OSD ? 1 : osd->flag;
		d->osd_factor = osd->factor;
		d->osd_acc = d->osd.flag == 0;
	}
	if (lay) {
		if ((st = upload(d, lay_chk, &d->ly.chk)) || (st = upload(d, lay_nbr, &d->ly.nbr))) return fail_create(d, st, "");
		d->layered = true;
		d->n_layers = n_layers;
		d->h_layer_of = layer_of;
		d->h_lay_off = lay_off;
	}
	d->fht = fht;
	d->h_coff = coff; d->h_cvar = c_var; d->h_ch = c_h;
	d->h_mul.assign(gf_mul, gf_mul + (size_t)q * q);
	d->d_e2c_map = (int *)d->g.v_cpos;
	d->shape = shape;
	if (shape.has_ems_toff()) {
		// permutation offsets of the specialised EMS kernel: variable-domain symbol a of lane l -> byte offset of h*a in a q-vector
		std::vector<unsigned long long> toff((size_t)E * 64);
		for (int ce = 0; ce < E; ce++)
			for (int l = 0; l < 64; l++) {
				unsigned long long pk = 0;
				for (int i = 0; i < 4; i++) {
					const int a = 2 * l + (i & 1) + 128 * (i >> 1);
					pk |= (unsigned long long)(8u * gf_mul[(size_t)c_h[ce] * q + a]) << (16 * i);
				}
				toff[(size_t)ce * 64 + l] = pk;
			}
		if ((st = upload(d, toff, &d->g.ems_toff))) return fail_create(d, st, "");
	}
	if (shape.has_dv2_row()) {
		std::vector<int> row((size_t)M * 16);
		for (int m = 0; m < M; m++)
			for (int j = 0; j < 4; j++) {
				const int ce = coff[m] + j, n = c_var[ce], e = c_epos[ce], e0 = voff[n];
				row[(size_t)m * 16 + j] = n;
				row[(size_t)m * 16 + 4 + j] = v_cpos[e0];
				row[(size_t)m * 16 + 8 + j] = v_cpos[e0 + 1];
				row[(size_t)m * 16 + 12 + j] = e | ((e == e0) ? (int)0x80000000 : 0);
			}
		if ((st = upload(d, row, &d->g.dv2_row))) return fail_create(d, st, "");
	}
	if (shape.has_c_nbr()) {
		// fused small-field iteration: everything the variable-node stage of a check-major edge needs, in one 16-byte row
		// (variable degrees 2 and 3 only: the fused loaders add the second c2v vector unconditionally; a code with a degree-1
		// variable takes the separate variable-node launch, which handles any degree)
		std::vector<int> nbr((size_t)E * 4);
		for (int ce = 0; ce < E; ce++) {
			const int n = c_var[ce], e0 = voff[n], dv = voff[n + 1] - e0;
			for (int k = 0; k < 3; k++) nbr[(size_t)ce * 4 + k] = k < dv ? v_cpos[e0 + k] : -1;
			nbr[(size_t)ce * 4 + 3] = (c_epos[ce] == e0) ? 1 : 0;
		}
		if ((st = upload(d, nbr, &d->g.c_nbr))) return fail_create(d, st, "");
	}
	void *cnt = nullptr;
	if (hipMalloc(&cnt, 16) != hipSuccess) return fail_create(d, NBL_ERR_NOMEM, "hipMalloc failed");
	d->graph_allocs.push_back(cnt);
	d->w.n_done = (int *)cnt;
	d->w.n_act = (int *)cnt + 1;
	if (hipEventCreate(&d->ev[0]) != hipSuccess || hipEventCreate(&d->ev[1]) != hipSuccess) return fail_create(d, NBL_ERR_HIP, "hipEventCreate failed");
	if (params->max_batch > 0 && (st = ensure_workspace(d, params->max_batch))) return fail_create(d, st, "");
	*out = d;
	return NBL_OK;
}

static void free_transmitter(nbl_decoder *d);

extern "C" void nbl_destroy(nbl_decoder *d)
{
	if (!d) return;
	if (d->device >= 0) (void)hipSetDevice(d->device);
	if (d->stream) { (void)hipStreamSynchronize(d->stream); }
	(void)hipDeviceSynchronize(); // graphs may still be running on a caller's stream
	free_workspace(d);
	for (void *p : d->graph_allocs) (void)hipFree(p);
	if (d->d_src) (void)hipFree(d->d_src);
	if (d->d_cons) (void)hipFree(d->d_cons);
	if (d->d_dmdesc) (void)hipFree(d->d_dmdesc);
	if (d->d_rx) (void)hipFree(d->d_rx);
	for (void *p : {(void *)d->d_tinv, (void *)d->d_prior, (void *)d->idd.rx[0], (void *)d->idd.rx[1], (void *)d->idd.idx[0], (void *)d->idd.idx[1],
	                (void *)d->idd.ext, (void *)d->idd.prior, (void *)d->idd.gain[0], (void *)d->idd.gain[1], (void *)d->d_gain, (void *)d->d_gains[0],
	                (void *)d->d_gains[1], (void *)d->d_jump_f, (void *)d->idd.res_out, (void *)d->idd.res_iters, (void *)d->idd.res_pass, (void *)d->idd.res_done})
		if (p) (void)hipFree(p);
	for (double *p : {d->d_lam, d->d_soft_sym, d->d_soft_bit})
		if (p) (void)hipFree(p);
	for (double *p : d->d_rxs)
		if (p) (void)hipFree(p);
	if (d->stream2) { (void)hipStreamSynchronize(d->stream2); (void)hipStreamDestroy(d->stream2); }
	for (void *p : {(void *)d->d_jump, (void *)d->d_state, (void *)d->d_txi, (void *)d->d_fn, (void *)d->d_fidx, (void *)d->d_farg, (void *)d->d_fval, (void *)d->d_fcount})
		if (p) (void)hipFree(p);
	for (void *p : {(void *)d->h_fidx, (void *)d->h_farg, (void *)d->h_fval})
		if (p) (void)hipHostFree(p);
	free_transmitter(d);
	for (auto &e : d->ev)
		if (e) (void)hipEventDestroy(e);
	if (d->h_ndone) (void)hipHostFree(d->h_ndone);
	for (auto &e : d->pev) (void)hipEventDestroy(e);
	if (d->stream) (void)hipStreamDestroy(d->stream);
	delete d;
}

extern "C" nbl_status nbl_set_profiling(nbl_decoder *d, int32_t on)
{
	if (!d) return NBL_ERR_ARG;
	d->profiling = on != 0;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): route every shape through the generic kernels.
extern "C" nbl_status nbl_debug_force_generic(nbl_decoder *d, int32_t on)
{
	if (!d) return NBL_ERR_ARG;
	d->force_generic = on;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): number of iteration windows currently held as executable hipGraphs
extern "C" int32_t nbl_debug_graph_windows(nbl_decoder *d)
{
	int n = 0;
	if (d)
		for (auto &ge : d->gexec) n += ge != nullptr;
	return n;
}

// Diagnostic only (not part of include/nbldpc.h): in-kernel cycle stamps of the check-node kernel.
extern "C" nbl_status nbl_debug_stamps(nbl_decoder *d, int32_t on, unsigned long long out[NBL_STAMP_SLOTS])
{
	if (!d) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	if (out && d->w.stamps) {
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		HIP_TRY(d, hipDeviceSynchronize());
		HIP_TRY(d, hipMemcpy(out, d->w.stamps, NBL_STAMP_SLOTS * 8, hipMemcpyDeviceToHost));
	}
	if (on && !d->w.stamps) {
		void *p = nullptr;
		HIP_TRY(d, hipMalloc(&p, NBL_STAMP_SLOTS * 8));
		d->graph_allocs.push_back(p);
		d->w.stamps = (unsigned long long *)p;
	}
	if (d->w.stamps && on) HIP_TRY(d, hipMemset(d->w.stamps, 0, NBL_STAMP_SLOTS * 8));
	if (!on) d->w.stamps = nullptr;
	return NBL_OK;
}

extern "C" nbl_status nbl_set_record_state(nbl_decoder *d, int32_t on)
{
	if (!d) return NBL_ERR_ARG;
	d->record_state = on != 0;
	return NBL_OK;
}

extern "C" nbl_status nbl_last_timing(nbl_decoder *d, double ms[4], int64_t launches[3])
{
	if (!d) return NBL_ERR_ARG;
	if (ms) memcpy(ms, d->ms, sizeof d->ms);
	if (launches) for (int i = 0; i < 3; i++) launches[i] = d->launches[i];
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): the kernel choice for a code description -- the shape and the plan, nothing else;
// no device, no decoder, no field tables.  layered_flags: NBL_LAYERED_* of nbl_create_layered_ex, -1 = the flooding schedule.
struct nbl_plan_info { const char *cn; int32_t fusable, fused, want_v2c; };
extern "C" nbl_status nbl_debug_plan(const nbl_code_desc *code, const nbl_params *params, const nbl_params_ext *ext, int32_t layered_flags,
                                     int32_t force_generic, int32_t record_state, nbl_plan_info *out)
{
	if (!code || !params || !out || code->N <= 0 || code->M <= 0) return NBL_ERR_ARG;
	const NblPlan plan = nbl_plan(nbl_shape(code), *params, ext ? *ext : nbl_params_ext{}, layered_flags >= 0, force_generic, record_state != 0, small_enabled());
	*out = {nbl_cn_name(plan.cn), plan.fusable, plan.fused, plan.want_v2c};
	return NBL_OK;
}

// The same for a decoder nbl_create_fht would make; fht_flags: NBL_FHT_* of include/nbldpc.h
extern "C" nbl_status nbl_debug_plan_fht(const nbl_code_desc *code, const nbl_params *params, uint32_t fht_flags, int32_t force_generic, int32_t record_state,
                                         nbl_plan_info *out)
{
	if (!code || !params || !out || code->N <= 0 || code->M <= 0) return NBL_ERR_ARG;
	const NblPlan plan = nbl_plan(nbl_shape(code), *params, nbl_params_ext{}, (fht_flags & NBL_FHT_LAYERED) != 0, force_generic, record_state != 0, small_enabled(), true);
	*out = {nbl_cn_name(plan.cn), plan.fusable, plan.fused, plan.want_v2c};
	return NBL_OK;
}

// The one launch of check-node kernel `cn`; fused: with the variable-node pass inside (w then carries c2v_prev).  The layered kernels
// run once per layer and are launched where the layers are walked (enqueue_window).
static nbl_status launch_cn(nbl_decoder *d, NblCn cn, const NblWork &w, const NblRun &r, bool fused, hipStream_t st)
{
	const NblGraphDev &g = d->g;
	switch (cn) {
	case NBL_CN_EMS256: HIP_TRY(d, nbl_launch_cn_ems256(g, w, r, fused, st)); break;
	case NBL_CN_EMS_SMALL: HIP_TRY(d, nbl_launch_cn_ems_small(g, w, r, fused, st)); break;
	case NBL_CN_EMS64: HIP_TRY(d, nbl_launch_cn_ems64(g, w, r, fused, st)); break;
	case NBL_CN_EMS: HIP_TRY(d, nbl_launch_cn_ems(g, w, r, st)); break;
	case NBL_CN_TEMS64: HIP_TRY(d, nbl_launch_cn_tems64(g, w, r, fused, st)); break;
	case NBL_CN_TEMS256: HIP_TRY(d, nbl_launch_cn_tems256(g, w, r, fused, st)); break;
	case NBL_CN_TEMS_SMALL: HIP_TRY(d, nbl_launch_cn_tems_small(g, w, r, fused, st)); break;
	case NBL_CN_TEMS: HIP_TRY(d, nbl_launch_cn_tems(g, w, r, st)); break;
	case NBL_CN_BP256: HIP_TRY(d, nbl_launch_cn_bp256(g, w, r, fused, st)); break;
	case NBL_CN_BP64: HIP_TRY(d, nbl_launch_cn_bp64(g, w, r, fused, st)); break;
	case NBL_CN_BP_SMALL: HIP_TRY(d, nbl_launch_cn_bp_small(g, w, r, fused, st)); break;
	case NBL_CN_BP: HIP_TRY(d, nbl_launch_cn_bp(g, w, r, st)); break;
	case NBL_CN_FHT: HIP_TRY(d, nbl_launch_cn_fht(g, w, r, st)); break;
	case NBL_CN_BSTEMS: HIP_TRY(d, nbl_launch_cn_bstems(g, w, r, st)); break;
	default: d->err = "check-node kernel for this method is not built yet"; return NBL_ERR_UNSUPPORTED;
	}
	return NBL_OK;
}

// The iteration loop of Decoding_BP / _EMS / _TEMS (NBLDPC.cpp:673 / 805 / 973): per iteration one fused launch + syndrome
// (specialised (2,4)-regular shapes) or the launch triple VN, syndrome, CN.  The launches of a window of iterations are captured
// into a hipGraph once and replayed (a decode is 100+ back-to-back launches: at small batches the gaps between them are most
// of the time).
struct IterCtx {
	nbl_decoder *d;
	NblPlan plan;
	NblRun r;
	bool damp;
	double *bufA, *bufB;
	const double *zeros = nullptr; // stands in for bufA in iteration 1 (then bufA needs no clearing)
	int batch = 0;                 // codewords of the call (r.B may shrink to the active list; the OSD sums cover every codeword)
	// profiling: one event after every launch on the launch stream; phase time = sum of the gaps it closes
	size_t nev = 0;
	std::vector<int> tag; // 0 vn, 1 syn, 2 cn, 3 other
};

static hipError_t mark(IterCtx &c, int t, hipStream_t st)
{
	nbl_decoder *d = c.d;
	if (!d->profiling) return hipSuccess;
	if (c.nev == d->pev.size()) { hipEvent_t e; hipError_t rc = hipEventCreate(&e); if (rc != hipSuccess) return rc; d->pev.push_back(e); }
	c.tag.push_back(t);
	return hipEventRecord(d->pev[c.nev++], st);
}

// launches of iterations it_lo .. it_hi on `st`
static nbl_status enqueue_window(IterCtx &c, int it_lo, int it_hi, hipStream_t st, bool count)
{
	nbl_decoder *d = c.d;
	for (int it = it_lo; it <= it_hi; it++) {
		c.r.iter = it;
		if (d->layered) {
			// decision and syndrome from the c2v the previous iteration left, then the layers in order, each on the c2v the layers
			// before it have just written (one buffer; the launches of a stream run in order)
			HIP_TRY(d, nbl_launch_vn_decide(d->g, d->w, c.r, st));
			HIP_TRY(d, mark(c, 0, st));
			HIP_TRY(d, nbl_launch_syn(d->g, d->w, c.r, st));
			HIP_TRY(d, mark(c, 1, st));
			// (T-EMS, log-QSPA: each check also damps its inputs against the v2c buffer and updates it in place; init_kernel has set
			// v2c = L_ch)
			for (int l = 0; l < d->n_layers; l++) {
				const int off = d->h_lay_off[l], cnt = d->h_lay_off[l + 1] - off;
				switch (c.plan.cn) {
				case NBL_CN_EMS_LAYERED: HIP_TRY(d, nbl_launch_cn_ems_layered(d->g, d->w, c.r, d->ly, off, cnt, st)); break;
				case NBL_CN_TEMS_LAYERED: HIP_TRY(d, nbl_launch_cn_tems_layered(d->g, d->w, c.r, d->ly, off, cnt, st)); break;
				case NBL_CN_BP_LAYERED: HIP_TRY(d, nbl_launch_cn_bp_layered(d->g, d->w, c.r, d->ly, off, cnt, st)); break;
				case NBL_CN_FHT_LAYERED: HIP_TRY(d, nbl_launch_cn_fht_layered(d->g, d->w, c.r, d->ly, off, cnt, st)); break;
				default: d->err = "layered schedule: no layered check-node kernel for this method"; return NBL_ERR_UNSUPPORTED;
				}
			}
			HIP_TRY(d, mark(c, 2, st));
			if (count) { d->launches[0]++; d->launches[1]++; d->launches[2] += d->n_layers; }
			continue;
		}
		if (c.plan.fused) {
			// one launch = variable-node pass + check-node pass; c2v ping-pongs between the two buffers
			NblWork wf = d->w;
			wf.c2v_prev = (it == 1 && c.zeros) ? c.zeros : (it & 1) ? c.bufA : c.bufB;
			wf.c2v_prev_shared = (it == 1 && c.zeros) ? 1 : 0;
			wf.c2v = (it & 1) ? c.bufB : c.bufA;
			wf.store_v2c = d->record_state ? 1 : 0;
			const nbl_status s = launch_cn(d, c.plan.cn, wf, c.r, true, st);
			if (s) return s;
			HIP_TRY(d, mark(c, 2, st));
			if (d->osd_acc) {
				HIP_TRY(d, nbl_launch_osd_acc(d->w.post, d->osd_S, c.batch, d->g.N, d->g.p, d->g.q, d->osd_factor, it == 1, st));
				HIP_TRY(d, mark(c, 3, st));
			}
			HIP_TRY(d, nbl_launch_syn(d->g, d->w, c.r, st));
			HIP_TRY(d, mark(c, 1, st));
			if (count) { d->launches[2]++; d->launches[1]++; }
			continue;
		}
		HIP_TRY(d, nbl_launch_vn(d->g, d->w, c.r, c.damp, st));
		HIP_TRY(d, mark(c, 0, st));
		if (d->osd_acc) {
			HIP_TRY(d, nbl_launch_osd_acc(d->w.post, d->osd_S, c.batch, d->g.N, d->g.p, d->g.q, d->osd_factor, it == 1, st));
			HIP_TRY(d, mark(c, 3, st));
		}
		HIP_TRY(d, nbl_launch_syn(d->g, d->w, c.r, st));
		HIP_TRY(d, mark(c, 1, st));
		if (count) { d->launches[0]++; d->launches[1]++; }
		// (the reference leaves the loop after the syndrome check of the last iteration it runs; the check-node pass of a
		// window's last iteration is only needed if another window follows -- it is cheap to keep the windows uniform)
		const nbl_status s = launch_cn(d, c.plan.cn, d->w, c.r, false, st);
		if (s) return s;
		HIP_TRY(d, mark(c, 2, st));
		if (count) d->launches[2]++;
	}
	return NBL_OK;
}

// Run window number `widx` (iterations it_lo..it_hi): replay its graph, capturing it first if needed; plain launches when
// graphs are off, while profiling (events between the launches) or if the capture fails.
static nbl_status run_window(IterCtx &c, int widx, int it_lo, int it_hi, hipStream_t st)
{
	nbl_decoder *d = c.d;
	const bool graph_ok = d->use_graph && !d->profiling && !d->w.stamps;
	if (graph_ok) {
		if ((int)d->gexec.size() <= widx) d->gexec.resize(widx + 1, nullptr);
		if (!d->gexec[widx]) {
			hipGraph_t graph = nullptr;
			if (hipStreamBeginCapture(d->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
				const nbl_status s = enqueue_window(c, it_lo, it_hi, d->stream, false);
				const hipError_t e = hipStreamEndCapture(d->stream, &graph);
				if (s == NBL_OK && e == hipSuccess && graph) {
					if (hipGraphInstantiate(&d->gexec[widx], graph, nullptr, nullptr, 0) != hipSuccess) d->gexec[widx] = nullptr;
				}
				if (graph) (void)hipGraphDestroy(graph);
				(void)hipGetLastError();
			}
			if (!d->gexec[widx]) d->use_graph = false; // capture is not available here: plain launches from now on
		}
		if (d->gexec[widx]) {
			HIP_TRY(d, hipGraphLaunch(d->gexec[widx], st));
			const int n = it_hi - it_lo + 1;
			d->launches[1] += n; d->launches[2] += d->layered ? (long long)n * d->n_layers : n;
			if (!c.plan.fused) d->launches[0] += n;
			return NBL_OK;
		}
	}
	return enqueue_window(c, it_lo, it_hi, st, true);
}

static nbl_status run_iterations(nbl_decoder *d, const double *d_Lin, int B, hipStream_t st)
{
	const nbl_params &p = d->prm;
	IterCtx c;
	c.d = d;
	d->idd_sub = false; // (the loop sets it again after its last pass)
	c.damp = p.method != NBL_METHOD_EMS;
	NblRun &r = c.r;
	r = NblRun{};
	r.B = B;
	r.fixed_iters = p.fixed_iters;
	if (p.method == NBL_METHOD_EMS) { r.nm = p.ems_nm; r.nc = p.ems_nc; r.factor = p.ems_factor; r.offset = p.ems_offset; }
	else if (p.method == NBL_METHOD_BS_TEMS) { r.nm = d->ext.bs_nm; r.nc = d->ext.bs_nc; r.factor = d->ext.bs_factor; r.offset = d->ext.bs_offset; }
	else { r.nr = p.tems_nr; r.nc = p.tems_nc; r.factor = p.tems_factor; r.offset = p.tems_offset; }
	r.damp_old = (p.method == NBL_METHOD_BP) ? 0.5 : 0.25;  // NBLDPC.cpp:739 / :1046 / :1262
	r.damp_new = (p.method == NBL_METHOD_BP) ? 0.5 : 0.75;
	d->launches[0] = d->launches[1] = d->launches[2] = 0;
	c.plan = plan_of(d); // (ensure_workspace has made c2v_alt and c2v_zero for every fusable shape)
	c.bufA = d->w.c2v;
	c.bufB = d->c2v_alt;
	c.zeros = c.plan.fused ? d->c2v_zero : nullptr;
	// the captured graphs hold buffer addresses and the batch size: any change drops them
	const nbl_decoder::GraphKey key = {d_Lin, d->w.Lch, d->w.v2c, d->w.c2v, d->c2v_alt, d->w.post, d->osd_S, B, d->record_state ? 1 : 0, d->force_generic, c.plan.fused ? 1 : 0};
	c.batch = B;
	if (memcmp(&key, &d->gkey, sizeof key) != 0) { drop_graphs(d); d->gkey = key; }
	HIP_TRY(d, mark(c, 3, st));
	HIP_TRY(d, nbl_launch_init(d_Lin, d->g, d->w, B, (c.damp ? 1 : 0) | (c.zeros ? 2 : 0), st)); // bit 1: c2v is not cleared
	HIP_TRY(d, mark(c, 3, st));
	d->last_c2v = c.zeros ? c.zeros : c.bufA;
	d->last_fused = c.plan.fused;
	// windows: fixed iterations or no polling -> one window; early exit -> `poll_every` iterations, then ask the device
	const bool polling = !p.fixed_iters && p.poll_every > 0;
	const int wlen = polling ? p.poll_every : (p.max_iter > 0 ? p.max_iter : 1);
	int last_it = 0;
	if (polling && !d->h_ndone) HIP_TRY(d, hipHostMalloc((void **)&d->h_ndone, 2 * sizeof(int), hipHostMallocDefault));
	// Early exit without idling the GPU: window w+1 is queued BEFORE the host looks at the count of converged codewords that
	// window w left behind (read back through pinned memory behind an event).  If everything had converged, the extra window
	// finds every codeword frozen and its kernels return at once; outputs, flags and iteration counts are unaffected.
	// Large batches: after every window the device rebuilds the list of codewords still iterating, and the grids of the next
	// windows cover that list -- sized by the newest converged count the host has seen, an upper bound of the list's length --
	// instead of the whole batch (most codewords of a waterfall batch are done long before the stragglers).
	const bool compact = polling && d->use_compact && !d->use_graph && B >= 1024;
	d->w.active = nullptr;
	int pending = -1; // parity of the read-back that has not been looked at yet
	const int max_iter = p.method == NBL_METHOD_OSD ? 0 : p.max_iter; // (method 6: Decoding_OSD_bit alone, no iterations)
	for (int it_lo = 1, widx = 0; it_lo <= max_iter; it_lo += wlen, widx++) {
		const int it_hi = (it_lo + wlen - 1 < p.max_iter) ? it_lo + wlen - 1 : p.max_iter;
		nbl_status s = run_window(c, widx, it_lo, it_hi, st);
		if (s) { d->w.active = nullptr; return s; }
		last_it = it_hi;
		if (polling) {
			const int par = widx & 1;
			HIP_TRY(d, hipMemcpyAsync(&d->h_ndone[par], d->w.n_done, sizeof(int), hipMemcpyDeviceToHost, st));
			HIP_TRY(d, hipEventRecord(d->ev[par], st));
			if (compact) {
				HIP_TRY(d, nbl_launch_compact(d->w.done, B, d->d_active, (int *)d->w.n_act, st));
				d->w.active = d->d_active;
			}
			if (pending >= 0) {
				HIP_TRY(d, hipEventSynchronize(d->ev[pending]));
				if (d->h_ndone[pending] >= B) break;
				if (compact) c.r.B = B - d->h_ndone[pending];
			}
			pending = par;
		}
	}
	d->w.active = nullptr;
	// OSD on every codeword that did not converge (NBLDPC.cpp:769-775: only after at least one iteration), or the whole of method 6
	if (d->osd_on && (p.method == NBL_METHOD_OSD || p.max_iter > 0)) {
		NblOsdDev o = d->osd;
		o.S = d->osd_S;
		HIP_TRY(d, nbl_launch_osd(d->g, d->w, o, B, st));
		HIP_TRY(d, mark(c, 3, st));
	}
	if (polling) HIP_TRY(d, hipStreamSynchronize(st));
	if (c.plan.fused && last_it > 0) d->last_c2v = (last_it & 1) ? c.bufB : c.bufA;
	if (d->profiling && c.nev > 0) {
		HIP_TRY(d, hipEventSynchronize(d->pev[c.nev - 1]));
		d->ms[0] = d->ms[1] = d->ms[2] = d->ms[3] = 0;
		for (size_t i = 1; i < c.nev; i++) {
			float ms = 0;
			HIP_TRY(d, hipEventElapsedTime(&ms, d->pev[i - 1], d->pev[i]));
			if (c.tag[i] < 3) d->ms[c.tag[i]] += ms;
			d->ms[3] += ms;
		}
	}
	d->last_B = B;
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_device(nbl_decoder *d, const double *d_L_ch, int32_t B, int32_t *d_out_sym,
                                              uint8_t *d_converged, int32_t *d_iters, void *stream)
{
	if (!d || !d_L_ch || !d_out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	hipStream_t st = stream ? (hipStream_t)stream : d->stream;
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	if ((s = run_iterations(d, d_L_ch, B, st))) return s;
	HIP_TRY(d, hipMemcpyAsync(d_out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToDevice, st));
	if (d_converged) HIP_TRY(d, hipMemcpyAsync(d_converged, d->w.done, (size_t)B, hipMemcpyDeviceToDevice, st));
	if (d_iters) HIP_TRY(d, hipMemcpyAsync(d_iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch(nbl_decoder *d, const double *L_ch, int32_t B, int32_t *out_sym, uint8_t *converged,
                                       int32_t *iters)
{
	if (!d || !L_ch || !out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	const size_t in_bytes = (size_t)B * d->g.N * (d->g.q - 1) * 8;
	if (!d->d_Lin) HIP_TRY(d, hipMalloc((void **)&d->d_Lin, (size_t)d->cap * d->g.N * (d->g.q - 1) * 8));
	HIP_TRY(d, hipMemcpyAsync(d->d_Lin, L_ch, in_bytes, hipMemcpyHostToDevice, d->stream));
	if ((s = run_iterations(d, d->d_Lin, B, d->stream))) return s;
	HIP_TRY(d, hipMemcpyAsync(out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->w.done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

// The per-symbol descriptor of the general demodulator (nbl_common.h, NblDemodPoint) from src [N p]; every index is checked here,
// before anything is indexed by it.
static nbl_status build_demod_desc(nbl_decoder *d, const nbl_demod_desc *dm, int m, std::vector<NblDemodPoint> &desc, std::vector<int> &tinv)
{
	const int N = d->g.N, p = d->g.p;
	const long long T = (long long)dm->n_mod_sym * m;
	std::vector<uint8_t> seen((size_t)T, 0);
	for (size_t i = 0; i < (size_t)N * p; i++) {
		const int t = dm->src[i];
		if (t < 0) continue;
		if (t >= T) { d->err = "demodulator source index out of range (label bit " + std::to_string(t) + " of code bit " + std::to_string(i) + ", L * m = " + std::to_string(T) + ")"; return NBL_ERR_ARG; }
		if (seen[t]) { d->err = "demodulator source: label bit " + std::to_string(t) + " is claimed twice"; return NBL_ERR_ARG; }
		seen[t] = 1;
	}
	tinv.assign((size_t)T, -1); // the inverse of src, for the prior-aware kernel: who claims label bit t
	for (size_t i = 0; i < (size_t)N * p; i++)
		if (dm->src[i] >= 0) tinv[dm->src[i]] = (int)i;
	NblDemodPoint none{};
	none.s = 0; none.nown = 0;
	for (int i = 0; i < 8; i++) none.own[i] = -1;
	desc.assign((size_t)N * (p + 1), none);
	for (int n = 0; n < N; n++) {
		NblDemodPoint *e = &desc[(size_t)n * (p + 1)];
		int pts[8], nt = 0;
		for (int j = 0; j < p; j++) {
			const int t = dm->src[(size_t)n * p + j];
			if (t < 0) continue;
			const int s = t / m;
			int k = 0;
			while (k < nt && pts[k] != s) k++;
			if (k == nt) pts[nt++] = s;
		}
		for (int x = 1; x < nt; x++) // ascending s
			for (int y = x; y > 0 && pts[y - 1] > pts[y]; y--) { const int tmp = pts[y]; pts[y] = pts[y - 1]; pts[y - 1] = tmp; }
		e[0].s = nt;
		for (int k = 0; k < nt; k++) e[1 + k].s = pts[k];
		for (int j = 0; j < p; j++) {
			const int t = dm->src[(size_t)n * p + j];
			if (t < 0) continue;
			int k = 0;
			while (pts[k] != t / m) k++;
			e[1 + k].own[t % m] = (int8_t)j;
			e[1 + k].nown++;
		}
	}
	return NBL_OK;
}

extern "C" nbl_status nbl_set_demodulator_ex(nbl_decoder *d, const nbl_demod_desc *dm, const nbl_demod_ext *ext)
{
	if (!d || !dm || !dm->src) return NBL_ERR_ARG;
	const int q = d->g.q, N = d->g.N, p = d->g.p;
	const int M = dm->mod_order;
	// every refusal comes before the device and the handle's state are touched: the demodulator set before stays usable
	if (M < 2 || M > 256 || (M & (M - 1))) {
		d->err = "nbl_set_demodulator: mod_order " + std::to_string(M) + " is not a power of two in 2 .. 256";
		return NBL_ERR_ARG;
	}
	const int metric = ext ? ext->metric : NBL_DEMOD_LOGSUM;
	if (metric != NBL_DEMOD_LOGSUM && metric != NBL_DEMOD_MAXLOG) {
		d->err = "nbl_set_demodulator_ex: unknown metric " + std::to_string(metric) + " (NBL_DEMOD_LOGSUM = 0, NBL_DEMOD_MAXLOG = 1)";
		return NBL_ERR_ARG;
	}
	const bool general = (M != 2 && M != q) || (ext && ext->force_general);
	if (dm->n_mod_sym <= 0) { d->err = "nbl_set_demodulator: n_mod_sym must be positive"; return NBL_ERR_ARG; }
	if ((general || M == q) && !dm->constellation) {
		d->err = "nbl_set_demodulator: this modulation order needs the constellation points (nbl_demod_desc.constellation)";
		return NBL_ERR_ARG;
	}
	const int m = ilog2(M);
	const size_t nsrc = (general || M == 2) ? (size_t)N * p : (size_t)N;
	std::vector<NblDemodPoint> desc;
	std::vector<int> tinv;
	if (general) {
		const nbl_status s = build_demod_desc(d, dm, m, desc, tinv);
		if (s) return s;
	} else {
		for (size_t i = 0; i < nsrc; i++)
			if (dm->src[i] >= dm->n_mod_sym) { d->err = "demodulator source index out of range"; return NBL_ERR_ARG; }
	}
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	free_transmitter(d); // its geometry repeats the demodulator's: set it again afterwards
	d->dm_order = 0;     // nothing is set until everything below has succeeded
	if (d->d_src) (void)hipFree(d->d_src);
	if (d->d_cons) (void)hipFree(d->d_cons);
	if (d->d_dmdesc) (void)hipFree(d->d_dmdesc);
	if (d->d_tinv) (void)hipFree(d->d_tinv);
	d->d_src = nullptr; d->d_cons = nullptr; d->d_dmdesc = nullptr; d->d_tinv = nullptr;
	if (general) {
		HIP_TRY(d, hipMalloc((void **)&d->d_dmdesc, desc.size() * sizeof(NblDemodPoint)));
		HIP_TRY(d, hipMemcpy(d->d_dmdesc, desc.data(), desc.size() * sizeof(NblDemodPoint), hipMemcpyHostToDevice));
		HIP_TRY(d, hipMalloc((void **)&d->d_tinv, tinv.size() * sizeof(int)));
		HIP_TRY(d, hipMemcpy(d->d_tinv, tinv.data(), tinv.size() * sizeof(int), hipMemcpyHostToDevice));
	} else {
		HIP_TRY(d, hipMalloc((void **)&d->d_src, nsrc * 4));
		HIP_TRY(d, hipMemcpy(d->d_src, dm->src, nsrc * 4, hipMemcpyHostToDevice));
	}
	d->h_cons.clear();
	if (dm->constellation) { // (BPSK: the demodulator does not need the points, the channel does)
		d->h_cons.assign(dm->constellation, dm->constellation + (size_t)2 * M);
		HIP_TRY(d, hipMalloc((void **)&d->d_cons, (size_t)M * 16));
		HIP_TRY(d, hipMemcpy(d->d_cons, dm->constellation, (size_t)M * 16, hipMemcpyHostToDevice));
	}
	// the channel's buffers are sized per lane of dm_L symbols and the jump table is per symbol position: both are rebuilt for
	// the new L by the next channel call
	if (d->d_jump) { (void)hipFree(d->d_jump); d->d_jump = nullptr; }
	if (d->d_jump_f) { (void)hipFree(d->d_jump_f); d->d_jump_f = nullptr; }
	d->jump_f_pos = 0;
	d->noise_cap = 0;
	d->noise_pos = 0;
	d->dm_general = general;
	d->dm_metric = metric;
	d->dm_order = M;
	d->dm_L = dm->n_mod_sym;
	return NBL_OK;
}

extern "C" nbl_status nbl_set_demodulator(nbl_decoder *d, const nbl_demod_desc *dm) { return nbl_set_demodulator_ex(d, dm, nullptr); }

// received samples -> L_ch in the workspace: the BPSK / q-ary kernel, or the general one where nbl_set_demodulator_ex chose it
// d_prior [B][N p] (may be NULL): the prior-aware instance of the general kernel; the BPSK / q-ary kernels have no foreign position, a
// prior is inert there
// d_gain [B][L][2] (may be NULL): the gain-aware instances of either kernel
static hipError_t launch_demod(nbl_decoder *d, const double *d_rx, double sigma, int B, const double *d_prior = nullptr, const double *d_gain = nullptr)
{
	if (d->dm_general)
		return nbl_launch_demod_general(d_rx, d->dm_L, sigma, d->dm_order, d->dm_metric, d->d_cons, d->d_dmdesc, d->g, d->w, B, d->stream, d_prior, d->d_tinv, d_gain);
	return nbl_launch_demod(d_rx, d->dm_L, sigma, d->dm_order, d->d_cons, d->d_src, d->g, d->w, B, d->stream, d_gain);
}

static nbl_status run_iterations(nbl_decoder *d, const double *d_Lin, int B, hipStream_t st);

template <typename T> static nbl_status grow_staging(nbl_decoder *d, T **buf, size_t *cap, size_t bytes);

// host samples [B][L][2] -> d_rx (grown on demand), on the decoder's stream
static nbl_status stage_rx(nbl_decoder *d, const double *rx, int B)
{
	const size_t bytes = (size_t)B * d->dm_L * 16;
	if (bytes > d->d_rx_cap) {
		if (d->d_rx) (void)hipFree(d->d_rx);
		d->d_rx = nullptr;
		d->d_rx_cap = 0;
		HIP_TRY(d, hipMalloc((void **)&d->d_rx, bytes));
		d->d_rx_cap = bytes;
	}
	HIP_TRY(d, hipMemcpyAsync(d->d_rx, rx, bytes, hipMemcpyHostToDevice, d->stream));
	d->rx_gain = false;
	return NBL_OK;
}

// a gain buffer grown on demand; its capacity is counted in nbl_workspace_bytes (the slots' are grown on the channel thread: each has
// its own counter, nothing shared is touched)
static nbl_status grow_gain(std::string &err, double **buf, size_t *cap, size_t bytes)
{
	if (bytes <= *cap) return NBL_OK;
	if (*buf) (void)hipFree(*buf);
	*buf = nullptr;
	*cap = 0;
	HIP_TRY_E(err, hipMalloc((void **)buf, bytes));
	*cap = bytes;
	return NBL_OK;
}

// host gains [B][L][2] -> d_gain, on the decoder's stream
static nbl_status stage_gain(nbl_decoder *d, const double *gain, int B)
{
	const size_t bytes = (size_t)B * d->dm_L * 16;
	if (nbl_status s = grow_gain(d->err, &d->d_gain, &d->d_gain_cap, bytes)) return s;
	HIP_TRY(d, hipMemcpyAsync(d->d_gain, gain, bytes, hipMemcpyHostToDevice, d->stream));
	d->rx_gain = true;
	return NBL_OK;
}

// nbl_decode_batch_samples, with a prior nbl_decode_batch_samples_prior, with gains nbl_decode_batch_samples_csi
static nbl_status decode_samples(nbl_decoder *d, const double *rx, const double *prior, double sigma, int32_t B, int32_t *out_sym,
                                 uint8_t *converged, int32_t *iters, const double *gain = nullptr)
{
	if (!d || !rx || !out_sym || B < 0 || !(sigma > 0)) return NBL_ERR_ARG;
	if (!d->dm_order) { d->err = "nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	if ((s = stage_rx(d, rx, B))) return s;
	if (gain && (s = stage_gain(d, gain, B))) return s;
	const double *d_gain = gain ? d->d_gain : nullptr;
	if (prior && d->dm_general) {
		const size_t pbytes = (size_t)B * d->g.N * d->g.p * 8;
		if ((s = grow_staging(d, &d->d_prior, &d->d_prior_cap, pbytes))) return s;
		HIP_TRY(d, hipMemcpyAsync(d->d_prior, prior, pbytes, hipMemcpyHostToDevice, d->stream));
		HIP_TRY(d, launch_demod(d, d->d_rx, sigma, B, d->d_prior, d_gain));
	} else {
		HIP_TRY(d, launch_demod(d, d->d_rx, sigma, B, nullptr, d_gain));
	}
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	HIP_TRY(d, hipMemcpyAsync(out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->w.done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_samples(nbl_decoder *d, const double *rx, double sigma, int32_t B, int32_t *out_sym,
                                               uint8_t *converged, int32_t *iters)
{
	return decode_samples(d, rx, nullptr, sigma, B, out_sym, converged, iters);
}

extern "C" nbl_status nbl_decode_batch_samples_prior(nbl_decoder *d, const double *rx, const double *prior, double sigma, int32_t B,
                                                     int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	return decode_samples(d, rx, prior, sigma, B, out_sym, converged, iters);
}

extern "C" nbl_status nbl_decode_batch_samples_csi(nbl_decoder *d, const double *rx, const double *gain, const double *prior, double sigma, int32_t B,
                                                   int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	return decode_samples(d, rx, prior, sigma, B, out_sym, converged, iters, gain);
}

// ---- bit-LLR input and batched soft output (nbl_soft.hip) ------------------------------------------------

// a staging buffer grown on demand, like d_rx; counted in nbl_workspace_bytes from the moment it exists
template <typename T> static nbl_status grow_staging(nbl_decoder *d, T **buf, size_t *cap, size_t bytes)
{
	if (bytes <= *cap) return NBL_OK;
	if (*buf) (void)hipFree(*buf);
	*buf = nullptr;
	d->soft_bytes -= *cap;
	*cap = 0;
	HIP_TRY(d, hipMalloc((void **)buf, bytes));
	*cap = bytes;
	d->soft_bytes += bytes;
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_bits_device(nbl_decoder *d, const double *d_bit_llr, int32_t B, int32_t *d_out_sym,
                                                   uint8_t *d_converged, int32_t *d_iters, void *stream)
{
	if (!d || !d_bit_llr || !d_out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	hipStream_t st = stream ? (hipStream_t)stream : d->stream;
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	HIP_TRY(d, nbl_launch_bits_to_lch(d_bit_llr, d->g, d->w, B, st));
	if ((s = run_iterations(d, nullptr, B, st))) return s; // (L_ch is in place: init_kernel leaves it alone)
	HIP_TRY(d, hipMemcpyAsync(d_out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToDevice, st));
	if (d_converged) HIP_TRY(d, hipMemcpyAsync(d_converged, d->w.done, (size_t)B, hipMemcpyDeviceToDevice, st));
	if (d_iters) HIP_TRY(d, hipMemcpyAsync(d_iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_bits(nbl_decoder *d, const double *bit_llr, int32_t B, int32_t *out_sym, uint8_t *converged,
                                            int32_t *iters)
{
	if (!d || !bit_llr || !out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	const size_t bytes = (size_t)B * d->g.N * d->g.p * 8;
	if ((s = grow_staging(d, &d->d_lam, &d->d_lam_cap, bytes))) return s;
	HIP_TRY(d, hipMemcpyAsync(d->d_lam, bit_llr, bytes, hipMemcpyHostToDevice, d->stream));
	HIP_TRY(d, nbl_launch_bits_to_lch(d->d_lam, d->g, d->w, B, d->stream));
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	HIP_TRY(d, hipMemcpyAsync(out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->w.done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): the batch size of the last decode call -- what nbl_soft_output's buffers are sized by
extern "C" int32_t nbl_debug_last_batch(const nbl_decoder *d) { return d ? d->last_B : 0; }

// what nbl_soft_output refuses, before the device is touched
static const char *const IDD_SUB_TEXT = ": the last decode call was an iterative-demapping loop (passes > 1), the workspace holds the "
                                        "sub-batch of its last pass and not the batch; run an ordinary decode call first";

static nbl_status soft_check(nbl_decoder *d, int32_t metric, uint32_t flags, const double *sym_llr, const double *bit_llr)
{
	if (!d) return NBL_ERR_ARG;
	if (d->prm.method == NBL_METHOD_OSD) { d->err = "nbl_soft_output: an OSD-only decoder (method 6) runs no iterations: there are no messages to form a posterior from"; return NBL_ERR_UNSUPPORTED; }
	if (!sym_llr && !bit_llr) { d->err = "nbl_soft_output: sym_llr and bit_llr are both NULL"; return NBL_ERR_ARG; }
	if (metric != NBL_SOFT_LOGSUM && metric != NBL_SOFT_MAXLOG) {
		d->err = "nbl_soft_output: unknown metric " + std::to_string(metric) + " (NBL_SOFT_LOGSUM = 0, NBL_SOFT_MAXLOG = 1)";
		return NBL_ERR_ARG;
	}
	if (flags & ~(uint32_t)NBL_SOFT_EXTRINSIC) {
		char hex[16];
		snprintf(hex, sizeof hex, "0x%x", (unsigned)(flags & ~(uint32_t)NBL_SOFT_EXTRINSIC));
		d->err = std::string("nbl_soft_output_ex: unknown flag bits ") + hex + " (NBL_SOFT_EXTRINSIC = 1)";
		return NBL_ERR_ARG;
	}
	if (d->last_B <= 0 || !d->w.Lch) { d->err = "nbl_soft_output: no decode call has run on this handle yet"; return NBL_ERR_ARG; }
	if (d->idd_sub) { d->err = std::string("nbl_soft_output") + IDD_SUB_TEXT; return NBL_ERR_ARG; }
	return NBL_OK;
}

// Where the c2v of the last decode call are: nbl_read_state's choice (below), handed to the kernel as a rule instead of being made per
// codeword on the host.
static NblSoftSrc soft_src(const nbl_decoder *d)
{
	NblSoftSrc s{};
	s.bufA = d->w.c2v;
	s.bufB = d->c2v_alt;
	s.zeros = d->c2v_zero;
	s.last = d->last_c2v ? d->last_c2v : d->w.c2v;
	s.last_shared = (d->c2v_zero && s.last == d->c2v_zero) ? 1 : 0;
	s.per_codeword = (d->last_fused && d->c2v_alt && !d->prm.fixed_iters) ? 1 : 0;
	s.done = d->w.done;
	s.iters = d->w.iters;
	return s;
}

extern "C" nbl_status nbl_soft_output_device_ex(nbl_decoder *d, int32_t metric, uint32_t flags, double *d_sym_llr, double *d_bit_llr, void *stream)
{
	nbl_status s = soft_check(d, metric, flags, d_sym_llr, d_bit_llr);
	if (s) return s;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	hipStream_t st = stream ? (hipStream_t)stream : d->stream;
	HIP_TRY(d, nbl_launch_soft_output(d->g, d->w.Lch, soft_src(d), d->last_B, metric, d_sym_llr, d_bit_llr, st, (flags & NBL_SOFT_EXTRINSIC) != 0));
	return NBL_OK;
}

extern "C" nbl_status nbl_soft_output_device(nbl_decoder *d, int32_t metric, double *d_sym_llr, double *d_bit_llr, void *stream)
{
	return nbl_soft_output_device_ex(d, metric, 0, d_sym_llr, d_bit_llr, stream);
}

extern "C" nbl_status nbl_soft_output_ex(nbl_decoder *d, int32_t metric, uint32_t flags, double *sym_llr, double *bit_llr)
{
	nbl_status s = soft_check(d, metric, flags, sym_llr, bit_llr);
	if (s) return s;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const size_t B = (size_t)d->last_B, N = d->g.N;
	const size_t sym_bytes = B * N * (d->g.q - 1) * 8, bit_bytes = B * N * d->g.p * 8;
	if (sym_llr && (s = grow_staging(d, &d->d_soft_sym, &d->d_soft_sym_cap, sym_bytes))) return s;
	if (bit_llr && (s = grow_staging(d, &d->d_soft_bit, &d->d_soft_bit_cap, bit_bytes))) return s;
	HIP_TRY(d, nbl_launch_soft_output(d->g, d->w.Lch, soft_src(d), d->last_B, metric, sym_llr ? d->d_soft_sym : nullptr,
	                                  bit_llr ? d->d_soft_bit : nullptr, d->stream, (flags & NBL_SOFT_EXTRINSIC) != 0));
	if (sym_llr) HIP_TRY(d, hipMemcpyAsync(sym_llr, d->d_soft_sym, sym_bytes, hipMemcpyDeviceToHost, d->stream));
	if (bit_llr) HIP_TRY(d, hipMemcpyAsync(bit_llr, d->d_soft_bit, bit_bytes, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_soft_output(nbl_decoder *d, int32_t metric, double *sym_llr, double *bit_llr)
{
	return nbl_soft_output_ex(d, metric, 0, sym_llr, bit_llr);
}

// ---- iterative demapping: the loop between the prior-aware demodulator and the decoder --------------------

// what the two _idd entry points refuse beyond what their plain forms refuse, before the device is touched
static nbl_status idd_check(nbl_decoder *d, const char *who, const nbl_idd_params *idd)
{
	const std::string w(who);
	if (!idd) { d->err = w + ": idd is NULL"; return NBL_ERR_ARG; }
	if (idd->passes < 1) { d->err = w + ": passes must be at least 1, got " + std::to_string(idd->passes); return NBL_ERR_ARG; }
	if (idd->soft_metric != NBL_SOFT_LOGSUM && idd->soft_metric != NBL_SOFT_MAXLOG) {
		d->err = w + ": unknown soft_metric " + std::to_string(idd->soft_metric) + " (NBL_SOFT_LOGSUM = 0, NBL_SOFT_MAXLOG = 1)";
		return NBL_ERR_ARG;
	}
	if (!d->dm_order) { d->err = w + ": nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (idd->passes > 1 && d->prm.method == NBL_METHOD_OSD) {
		d->err = w + ": an OSD-only decoder (method 6) runs no iterations: there are no messages to form a prior from, passes must be 1";
		return NBL_ERR_UNSUPPORTED;
	}
	return NBL_OK;
}

// passes 1 .. idd->passes over the samples d_rx0 [B][L][2] (only ever read); leaves out / converged / iters / pass of every codeword at
// its batch position in d->idd.res_*.  One stream synchronisation per pass that has a successor: the survivor count sizes the next grids.
// d_gain0 [B][L][2] (may be NULL): the gains of those samples; the survivors' rows are gathered with their samples.
static nbl_status run_idd(nbl_decoder *d, const double *d_rx0, double sigma, int B, const nbl_idd_params *idd, const double *d_gain0 = nullptr)
{
	nbl_decoder::Idd &x = d->idd;
	const int N = d->g.N, Np = d->g.N * d->g.p, rx_row = 2 * d->dm_L;
	nbl_status s;
	if ((s = grow_staging(d, &x.res_out, &x.out_cap, (size_t)B * N * 4))) return s;
	if ((s = grow_staging(d, &x.res_iters, &x.iters_cap, (size_t)B * 4))) return s;
	if ((s = grow_staging(d, &x.res_pass, &x.pass_cap, (size_t)B * 4))) return s;
	if ((s = grow_staging(d, &x.res_done, &x.done_cap, (size_t)B))) return s;
	const double *rx = d_rx0, *prior = nullptr, *gain = d_gain0;
	const int *idx = nullptr;
	int n = B, side = 0;
	for (int k = 1;; k++) {
		HIP_TRY(d, launch_demod(d, rx, sigma, n, prior, gain));
		if ((s = run_iterations(d, nullptr, n, d->stream))) return s;
		HIP_TRY(d, nbl_launch_idd_scatter(d->w.out, d->w.done, d->w.iters, idx, n, N, k, x.res_out, x.res_done, x.res_iters, x.res_pass, d->stream));
		if (k == idd->passes) break;
		int live = 0;
		HIP_TRY(d, nbl_launch_compact(d->w.done, n, d->d_active, (int *)d->w.n_act, d->stream));
		HIP_TRY(d, hipMemcpyAsync(&live, d->w.n_act, sizeof live, hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		if (live <= 0) break;
		if (live > n) { d->err = "iterative demapping: the active list is longer than the batch"; return NBL_ERR_HIP; }
		if ((s = grow_staging(d, &x.ext, &x.ext_cap, (size_t)n * Np * 8))) return s;
		if ((s = grow_staging(d, &x.prior, &x.prior_cap, (size_t)live * Np * 8))) return s;
		if ((s = grow_staging(d, &x.rx[side], &x.rx_cap[side], (size_t)live * rx_row * 8))) return s;
		if ((s = grow_staging(d, &x.idx[side], &x.idx_cap[side], (size_t)live * 4))) return s;
		HIP_TRY(d, nbl_launch_soft_output(d->g, d->w.Lch, soft_src(d), n, idd->soft_metric, nullptr, x.ext, d->stream, true));
		if (gain && (s = grow_staging(d, &x.gain[side], &x.gain_cap[side], (size_t)live * rx_row * 8))) return s;
		HIP_TRY(d, nbl_launch_idd_gather(d->d_active, live, rx, rx_row, x.ext, Np, idx, x.rx[side], x.prior, x.idx[side], d->stream, gain,
		                                 gain ? x.gain[side] : nullptr));
		rx = x.rx[side];
		if (gain) gain = x.gain[side];
		idx = x.idx[side];
		prior = x.prior;
		side ^= 1;
		n = live;
	}
	d->idd_sub = true;
	return NBL_OK;
}

// a demodulator without a foreign position (BPSK / q-ary, not forced general): every pass is the same decode, so pass 1 is run alone
// and a codeword that did not converge is reported with the pass the definition ends on
static void idd_inert_passes(const nbl_idd_params *idd, const uint8_t *conv, int32_t B, int32_t *passes_used)
{
	if (passes_used)
		for (int b = 0; b < B; b++) passes_used[b] = conv[b] ? 1 : idd->passes;
}

// nbl_decode_batch_samples_idd, with gains nbl_decode_batch_samples_idd_csi
static nbl_status decode_samples_idd(nbl_decoder *d, const char *who, const double *rx, const double *gain, double sigma, int32_t B,
                                     const nbl_idd_params *idd, int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used)
{
	if (!d || !rx || !out_sym || B < 0 || !(sigma > 0)) return NBL_ERR_ARG;
	nbl_status s = idd_check(d, who, idd);
	if (s) return s;
	if (B == 0) return NBL_OK;
	if (idd->passes == 1 || !d->dm_general) {
		std::vector<uint8_t> conv(converged ? 0 : (size_t)B);
		uint8_t *cv = converged ? converged : conv.data();
		if ((s = decode_samples(d, rx, nullptr, sigma, B, out_sym, cv, iters, gain))) return s;
		idd_inert_passes(idd, cv, B, passes_used);
		return NBL_OK;
	}
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	if ((s = ensure_workspace(d, B))) return s;
	if ((s = stage_rx(d, rx, B))) return s;
	if (gain && (s = stage_gain(d, gain, B))) return s;
	if ((s = run_idd(d, d->d_rx, sigma, B, idd, gain ? d->d_gain : nullptr))) return s;
	HIP_TRY(d, hipMemcpyAsync(out_sym, d->idd.res_out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->idd.res_done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->idd.res_iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	if (passes_used) HIP_TRY(d, hipMemcpyAsync(passes_used, d->idd.res_pass, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_samples_idd(nbl_decoder *d, const double *rx, double sigma, int32_t B, const nbl_idd_params *idd,
                                                   int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used)
{
	return decode_samples_idd(d, "nbl_decode_batch_samples_idd", rx, nullptr, sigma, B, idd, out_sym, converged, iters, passes_used);
}

extern "C" nbl_status nbl_decode_batch_samples_idd_csi(nbl_decoder *d, const double *rx, const double *gain, double sigma, int32_t B,
                                                       const nbl_idd_params *idd, int32_t *out_sym, uint8_t *converged, int32_t *iters,
                                                       int32_t *passes_used)
{
	return decode_samples_idd(d, gain ? "nbl_decode_batch_samples_idd_csi" : "nbl_decode_batch_samples_idd", rx, gain, sigma, B, idd, out_sym,
	                          converged, iters, passes_used);
}

// ---- AWGN channel + CRand on the device ------------------------------------------------------------------

static uint32_t mod_pow(uint32_t a, uint64_t k, uint32_t m)
{
	uint64_t r = 1 % m, x = a % m;
	for (; k; k >>= 1) {
		if (k & 1) r = r * x % m;
		x = x * x % m;
	}
	return (uint32_t)r;
}

extern "C" void nbl_rand_advance(uint32_t state[3], uint64_t draws)
{
	state[0] = (uint32_t)((uint64_t)(state[0] % 61967u) * mod_pow(249, draws, 61967) % 61967u);
	state[1] = (uint32_t)((uint64_t)(state[1] % 63443u) * mod_pow(251, draws, 63443) % 63443u);
	state[2] = (uint32_t)((uint64_t)(state[2] % 63599u) * mod_pow(252, draws, 63599) % 63599u);
}

// A^(4 k) mod m for k < npos, [3][npos]: the state in front of position k of a frame, as a factor on the lane's state
static std::vector<uint32_t> jump_table(size_t npos)
{
	std::vector<uint32_t> jump(3 * npos);
	const uint32_t A[3] = {249, 251, 252}, M[3] = {61967, 63443, 63599};
	for (int g = 0; g < 3; g++) {
		uint64_t x = 1;
		const uint32_t a4 = mod_pow(A[g], 4, M[g]);
		for (size_t s = 0; s < npos; s++) { jump[g * npos + s] = (uint32_t)x; x = x * a4 % M[g]; }
	}
	return jump;
}

// nblk of the fading frame at the current L (0 without fading): the frame has nblk + L positions of four uniform draws
static int fading_blocks(const nbl_decoder *d)
{
	return d->fade_model == NBL_FADING_RAYLEIGH ? (d->dm_L + d->fade_coh - 1) / d->fade_coh : 0;
}

static nbl_status ensure_noise(nbl_decoder *d, int B, std::string &err)
{
	const size_t nblk = (size_t)fading_blocks(d);
	const size_t L = (size_t)d->dm_L + nblk; // positions per lane: the buffers below are per position
	if (nblk && (!d->d_jump_f || d->jump_f_pos != (int)L)) { // the table of the fading frame, beside the AWGN one
		if (d->d_jump_f) (void)hipFree(d->d_jump_f);
		d->d_jump_f = nullptr;
		d->jump_f_pos = 0;
		const std::vector<uint32_t> jump = jump_table(L);
		HIP_TRY_E(err, hipMalloc((void **)&d->d_jump_f, jump.size() * 4));
		HIP_TRY_E(err, hipMemcpy(d->d_jump_f, jump.data(), jump.size() * 4, hipMemcpyHostToDevice));
		d->jump_f_pos = (int)L;
	}
	if (!nblk && !d->d_jump) {
		const std::vector<uint32_t> jump = jump_table(L);
		HIP_TRY_E(err, hipMalloc((void **)&d->d_jump, jump.size() * 4));
		HIP_TRY_E(err, hipMemcpy(d->d_jump, jump.data(), jump.size() * 4, hipMemcpyHostToDevice));
	}
	if ((size_t)B <= d->noise_cap && L <= d->noise_pos) return NBL_OK; // (capacity in lanes of noise_pos positions; nbl_set_demodulator resets it)
	for (void *p : {(void *)d->d_state, (void *)d->d_txi, (void *)d->d_fn, (void *)d->d_fidx, (void *)d->d_farg, (void *)d->d_fval})
		if (p) (void)hipFree(p);
	for (void *p : {(void *)d->h_fidx, (void *)d->h_farg, (void *)d->h_fval})
		if (p) (void)hipHostFree(p);
	d->d_state = nullptr; d->d_txi = nullptr; d->d_fn = nullptr; d->d_fidx = nullptr; d->d_farg = d->d_fval = nullptr;
	d->h_fidx = nullptr; d->h_farg = d->h_fval = nullptr;
	d->noise_cap = 0;
	d->noise_pos = 0;
	const size_t nval = (size_t)B * L * 4; // two functions per normal draw, two draws per symbol
	if (nval > 0xffffffffull) { err = "nbl_decode_batch_noise: batch * symbols too large for 32-bit value indices"; return NBL_ERR_ARG; }
	// about 16 % of the values are uncertain (5 % of the logarithms, 11 % of the cosines); room for 30 %
	const size_t cap = nval * 3 / 10 + 4096;
	HIP_TRY_E(err, hipMalloc((void **)&d->d_state, (size_t)B * 12));
	HIP_TRY_E(err, hipMalloc((void **)&d->d_txi, (size_t)B * L));
	HIP_TRY_E(err, hipMalloc((void **)&d->d_fn, nval * 8));
	HIP_TRY_E(err, hipMalloc((void **)&d->d_fidx, cap * 4));
	HIP_TRY_E(err, hipMalloc((void **)&d->d_farg, cap * 8));
	HIP_TRY_E(err, hipMalloc((void **)&d->d_fval, cap * 8));
	if (!d->d_fcount) HIP_TRY_E(err, hipMalloc((void **)&d->d_fcount, 16));
	HIP_TRY_E(err, hipHostMalloc((void **)&d->h_farg, cap * 8, hipHostMallocDefault));
	HIP_TRY_E(err, hipHostMalloc((void **)&d->h_fval, cap * 8, hipHostMallocDefault));
	d->noise_cap = B;
	d->noise_pos = L;
	d->flag_cap = cap;
	return NBL_OK;
}

// Forms RX = TX + noise for B lanes in *rx_buf (grown on demand) on stream `st`: the three kernels of nbl_noise.hip with the host's
// libm in between.  Returns with the samples complete in HBM.
// tx_index == NULL: the indices are already on the device, in d_txi_dev (nbl_transmit_batch).
// Under nbl_set_fading(RAYLEIGH) the generate kernel runs over the nblk + L positions of the fading frame and nbl_fading.hip's finish
// kernel forms RX = h * TX + noise, with the per-sample gains into *gain_buf (grown on demand); *has_gain says which of the two ran.
static nbl_status run_channel(nbl_decoder *d, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int B, hipStream_t st,
                              double **rx_buf, size_t *rx_cap, double **gain_buf, size_t *gain_cap, bool *has_gain, std::string &err,
                              const uint8_t *d_txi_dev = nullptr)
{
	*has_gain = false;
	if (!d->dm_order) { err = "nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (d->h_cons.empty() || !d->d_cons) { err = "the channel needs the constellation points (nbl_demod_desc.constellation), also for BPSK"; return NBL_ERR_ARG; }
	nbl_status s = ensure_noise(d, B, err);
	if (s) return s;
	const size_t L = d->dm_L;
	if (tx_index && d->dm_order < 256) { // an index beyond the constellation would read past d_cons in the finish kernel (8 bytes per step:
		// the modulation orders are powers of two, so "some byte >= order" is "some bit above the order's bits is set")
		const size_t n = (size_t)B * L;
		const uint8_t hi = (uint8_t)~(d->dm_order - 1);
		uint64_t m8 = 0, any = 0;
		for (int k = 0; k < 8; k++) m8 = (m8 << 8) | hi;
		size_t i = 0;
		for (; i + 8 <= n; i += 8) { uint64_t w8; memcpy(&w8, tx_index + i, 8); any |= w8 & m8; }
		for (; i < n; i++) any |= (uint64_t)(tx_index[i] & hi);
		if (any || (d->dm_order & (d->dm_order - 1))) {
			for (size_t k = 0; k < n; k++)
				if ((int)tx_index[k] >= d->dm_order) { err = "tx_index holds a value >= mod_order"; return NBL_ERR_ARG; }
		}
	}
	const size_t bytes = (size_t)B * L * 16;
	if (bytes > *rx_cap) {
		if (*rx_buf) (void)hipFree(*rx_buf);
		*rx_buf = nullptr;
		HIP_TRY_E(err, hipMalloc((void **)rx_buf, bytes));
		*rx_cap = bytes;
	}
	const int nblk = fading_blocks(d), npos = (int)L + nblk;
	if (nblk && (s = grow_gain(err, gain_buf, gain_cap, bytes))) return s;
	const bool timing = getenv("NBL_CHANNEL_TIMING") != nullptr;
	auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double t0 = now();
	double t1 = t0, t2 = t0, t3 = t0;
	HIP_TRY_E(err, hipMemcpyAsync(d->d_state, lane_state, (size_t)B * 12, hipMemcpyHostToDevice, st));
	if (tx_index) HIP_TRY_E(err, hipMemcpyAsync(d->d_txi, tx_index, (size_t)B * L, hipMemcpyHostToDevice, st));
	HIP_TRY_E(err, hipMemsetAsync(d->d_fcount, 0, 4, st));
	HIP_TRY_E(err, nbl_launch_noise_gen(d->d_state, nblk ? d->d_jump_f : d->d_jump, npos, B, d->d_fn, d->d_fidx, d->d_farg, d->d_fcount, (unsigned)d->flag_cap, st));
	unsigned nflag = 0;
	HIP_TRY_E(err, hipMemcpyAsync(&nflag, d->d_fcount, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY_E(err, hipStreamSynchronize(st));
	if (nflag > d->flag_cap) { err = "nbl_decode_batch_noise: more uncertain values than the list holds (30 % of all)"; return NBL_ERR_NOMEM; }
	d->last_flag_frac = (double)nflag / ((double)B * npos * 4);
	t1 = now();
	if (nflag) {
		HIP_TRY_E(err, hipMemcpyAsync(d->h_farg, d->d_farg, (size_t)nflag * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY_E(err, hipStreamSynchronize(st));
		t2 = now();
		// the host's own libm decides the uncertain values: log(1 - u1) or cos(2 pi u2), Rand.cpp:35
		int T = (int)std::thread::hardware_concurrency();
		if (const char *e = getenv("NBL_HOST_THREADS")) T = atoi(e);
		if (T > 16) T = 16;
		if (T < 1 || nflag < 4096) T = 1;
		auto work = [&](unsigned lo, unsigned hi) {
			// arguments of the logarithm are 1 - u1 in (0, 1]; arguments of the cosine are 2 pi u2 in [0, 2 pi): the list marks a
			// cosine argument by its sign bit (the kernel stores -x, and -0.0 for x = 0), so only the arguments travel
			for (unsigned k = lo; k < hi; k++) {
				const double a = d->h_farg[k];
				d->h_fval[k] = std::signbit(a) ? std::cos(-a) : std::log(a);
			}
		};
		if (T == 1) work(0, nflag);
		else {
			std::vector<std::thread> th;
			for (int t = 0; t < T; t++) th.emplace_back(work, (unsigned)((uint64_t)nflag * t / T), (unsigned)((uint64_t)nflag * (t + 1) / T));
			for (auto &x : th) x.join();
		}
		t3 = now();
		HIP_TRY_E(err, hipMemcpyAsync(d->d_fval, d->h_fval, (size_t)nflag * 8, hipMemcpyHostToDevice, st));
		HIP_TRY_E(err, nbl_launch_noise_patch(d->d_fn, d->d_fidx, d->d_fval, nflag, st));
	}
	if (nblk)
		HIP_TRY_E(err, nbl_launch_fading_finish(d->d_fn, tx_index ? d->d_txi : d_txi_dev, d->d_cons, sigma, (int)L, nblk, d->fade_coh, B, *rx_buf, *gain_buf, st));
	else
		HIP_TRY_E(err, nbl_launch_noise_finish(d->d_fn, tx_index ? d->d_txi : d_txi_dev, d->d_cons, sigma, (int)L, B, *rx_buf, st));
	HIP_TRY_E(err, hipStreamSynchronize(st));
	*has_gain = nblk != 0;
	if (timing)
		fprintf(stderr, "[channel] B=%d: generate %.2f ms, list to host %.2f ms, host libm (%u values) %.2f ms, patch + finish %.2f ms\n", B,
		        (t1 - t0) * 1e3, (t2 - t1) * 1e3, nflag, (t3 - t2) * 1e3, (now() - t3) * 1e3);
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_noise(nbl_decoder *d, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B,
                                             int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	if (!d || !tx_index || !lane_state || !out_sym || B < 0 || !(sigma > 0)) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	if ((s = run_channel(d, tx_index, lane_state, sigma, B, d->stream, &d->d_rx, &d->d_rx_cap, &d->d_gain, &d->d_gain_cap, &d->rx_gain, d->err))) return s;
	HIP_TRY(d, launch_demod(d, d->d_rx, sigma, B, nullptr, d->rx_gain ? d->d_gain : nullptr));
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	HIP_TRY(d, hipMemcpyAsync(out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->w.done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

// Two-phase form: the channel of batch k+1 (second stream, host libm) may run on another host thread while batch k is decoded.
extern "C" nbl_status nbl_channel_batch(nbl_decoder *d, int32_t slot, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B)
{
	if (!d || !tx_index || !lane_state || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	d->err2.clear();
	HIP_TRY_E(d->err2, hipSetDevice(d->device));
	if (!d->stream2) HIP_TRY_E(d->err2, hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking));
	d->rxs_B[slot] = 0;
	const nbl_status s = run_channel(d, tx_index, lane_state, sigma, B, d->stream2, &d->d_rxs[slot], &d->d_rxs_cap[slot], &d->d_gains[slot],
	                                 &d->d_gains_cap[slot], &d->slot_gain[slot], d->err2);
	if (s == NBL_OK) d->rxs_B[slot] = B;
	return s;
}

static nbl_status ensure_slot_dec(nbl_decoder *d, int slot, int B)
{
	const size_t need = (size_t)B * d->g.N * 4;
	if (need <= d->tx.dec_cap[slot]) return NBL_OK;
	if (d->tx.dec[slot]) (void)hipFree(d->tx.dec[slot]);
	d->tx.dec[slot] = nullptr;
	d->tx.dec_cap[slot] = 0;
	HIP_TRY(d, hipMalloc((void **)&d->tx.dec[slot], need));
	d->tx.dec_cap[slot] = need;
	return NBL_OK;
}

// what the two resident decode calls refuse about their slot and outputs
static nbl_status resident_check(nbl_decoder *d, int slot, int B, const int32_t *out_sym)
{
	if (!out_sym && !d->tx.on) { d->err = "nbl_decode_batch_resident: out_sym may only be NULL once nbl_set_transmitter has been called"; return NBL_ERR_ARG; }
	if (d->rxs_B[slot] != B) { d->err = "nbl_decode_batch_resident: slot does not hold the samples of a batch of this size (nbl_channel_batch first)"; return NBL_ERR_ARG; }
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_resident(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	if (!d || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	if (nbl_status rs = resident_check(d, slot, B, out_sym)) return rs;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	HIP_TRY(d, launch_demod(d, d->d_rxs[slot], sigma, B, nullptr, d->slot_gain[slot] ? d->d_gains[slot] : nullptr));
	if (d->tx.on) d->tx.dec_B[slot] = 0;
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	if (out_sym) HIP_TRY(d, hipMemcpyAsync(out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (d->tx.on) { // the slot keeps its outputs for nbl_count_errors
		if ((s = ensure_slot_dec(d, slot, B))) return s;
		HIP_TRY(d, hipMemcpyAsync(d->tx.dec[slot], d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToDevice, d->stream));
	}
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->w.done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	if (d->tx.on) d->tx.dec_B[slot] = B;
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_resident_idd(nbl_decoder *d, int32_t slot, double sigma, int32_t B, const nbl_idd_params *idd,
                                                    int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used)
{
	if (!d || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	nbl_status s = idd_check(d, "nbl_decode_batch_resident_idd", idd);
	if (s) return s;
	if (idd->passes == 1 || !d->dm_general) {
		std::vector<uint8_t> conv(converged ? 0 : (size_t)B);
		uint8_t *cv = converged ? converged : conv.data();
		if ((s = nbl_decode_batch_resident(d, slot, sigma, B, out_sym, cv, iters))) return s;
		idd_inert_passes(idd, cv, B, passes_used);
		return NBL_OK;
	}
	if (nbl_status rs = resident_check(d, slot, B, out_sym)) return rs;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	if ((s = ensure_workspace(d, B))) return s;
	if (d->tx.on) d->tx.dec_B[slot] = 0;
	if ((s = run_idd(d, d->d_rxs[slot], sigma, B, idd, d->slot_gain[slot] ? d->d_gains[slot] : nullptr))) return s; // (the slot's samples and gains are only read)
	if (out_sym) HIP_TRY(d, hipMemcpyAsync(out_sym, d->idd.res_out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (d->tx.on) { // the slot keeps the final words for nbl_count_errors
		if ((s = ensure_slot_dec(d, slot, B))) return s;
		HIP_TRY(d, hipMemcpyAsync(d->tx.dec[slot], d->idd.res_out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToDevice, d->stream));
	}
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->idd.res_done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->idd.res_iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	if (passes_used) HIP_TRY(d, hipMemcpyAsync(passes_used, d->idd.res_pass, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	if (d->tx.on) d->tx.dec_B[slot] = B;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): device time in milliseconds of ONE launch of the demodulator on the samples a slot
// holds, between two events on the decoder's stream -- with_prior != 0: the prior-aware instance, on an all-zero prior (the kernel's
// work does not depend on the values).  For tools/idd_pass.py.
// with_gain != 0 (nbl_debug_time_demod_csi): the gain-aware instance, on the slot's own gains where it holds some, else on all-zero
// gains (the kernel's work does not depend on the values).  For tools/fading_fer.py.
static nbl_status time_demod(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t with_prior, int32_t with_gain, double *ms)
{
	if (!d || !ms || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0) || !d->dm_order || d->rxs_B[slot] != B) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	const double *prior = nullptr;
	if (with_prior && d->dm_general) {
		const size_t pbytes = (size_t)B * d->g.N * d->g.p * 8;
		if ((s = grow_staging(d, &d->d_prior, &d->d_prior_cap, pbytes))) return s;
		HIP_TRY(d, hipMemsetAsync(d->d_prior, 0, pbytes, d->stream));
		prior = d->d_prior;
	}
	const double *gain = nullptr;
	if (with_gain && d->slot_gain[slot]) gain = d->d_gains[slot];
	else if (with_gain) {
		const size_t gbytes = (size_t)B * d->dm_L * 16;
		if ((s = grow_gain(d->err, &d->d_gain, &d->d_gain_cap, gbytes))) return s;
		HIP_TRY(d, hipMemsetAsync(d->d_gain, 0, gbytes, d->stream));
		d->rx_gain = false;
		gain = d->d_gain;
	}
	hipEvent_t a = nullptr, b = nullptr;
	HIP_TRY(d, hipEventCreate(&a));
	HIP_TRY(d, hipEventCreate(&b));
	hipError_t e = hipEventRecord(a, d->stream);
	if (e == hipSuccess) e = launch_demod(d, d->d_rxs[slot], sigma, B, prior, gain);
	if (e == hipSuccess) e = hipEventRecord(b, d->stream);
	if (e == hipSuccess) e = hipEventSynchronize(b);
	float t = 0;
	if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
	(void)hipEventDestroy(a);
	(void)hipEventDestroy(b);
	HIP_TRY(d, e);
	*ms = t;
	return NBL_OK;
}

extern "C" nbl_status nbl_debug_time_demod(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t with_prior, double *ms)
{
	return time_demod(d, slot, sigma, B, with_prior, 0, ms);
}

extern "C" nbl_status nbl_debug_time_demod_csi(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t with_prior, int32_t with_gain, double *ms)
{
	return time_demod(d, slot, sigma, B, with_prior, with_gain, ms);
}

// ---- flat fading (include/nbldpc.h) ---------------------------------------------------------------------------

extern "C" nbl_status nbl_set_fading(nbl_decoder *d, const nbl_fading_desc *f)
{
	if (!d) return NBL_ERR_ARG;
	if (!f || f->model == NBL_FADING_NONE) { d->fade_model = NBL_FADING_NONE; d->fade_coh = 1; return NBL_OK; }
	if (f->model != NBL_FADING_RAYLEIGH) {
		d->err = "nbl_set_fading: unknown model " + std::to_string(f->model) + " (NBL_FADING_NONE = 0, NBL_FADING_RAYLEIGH = 1)";
		return NBL_ERR_ARG;
	}
	if (f->coherence < 1) {
		d->err = "nbl_set_fading: coherence must be at least 1, got " + std::to_string(f->coherence);
		return NBL_ERR_ARG;
	}
	d->fade_model = f->model;
	d->fade_coh = f->coherence;
	return NBL_OK;
}

extern "C" uint64_t nbl_channel_draws(const nbl_decoder *d)
{
	return d ? 4ull * (uint64_t)fading_blocks(d) + 4ull * (uint64_t)d->dm_L : 0;
}

extern "C" nbl_status nbl_read_gains(nbl_decoder *d, int32_t slot, int32_t b0, int32_t n, double *gain)
{
	if (!d || slot < 0 || slot > 1 || b0 < 0 || n < 0 || (n > 0 && !gain)) return NBL_ERR_ARG;
	d->err.clear();
	if (d->rxs_B[slot] <= 0 || !d->slot_gain[slot]) { d->err = "nbl_read_gains: the slot holds no gains (its samples were not formed under nbl_set_fading)"; return NBL_ERR_ARG; }
	if ((long long)b0 + n > d->rxs_B[slot]) { d->err = "nbl_read_gains: the slot does not hold these lanes"; return NBL_ERR_ARG; }
	if (n == 0) return NBL_OK;
	HIP_TRY(d, hipSetDevice(d->device));
	HIP_TRY(d, hipMemcpy(gain, d->d_gains[slot] + (size_t)b0 * d->dm_L * 2, (size_t)n * d->dm_L * 16, hipMemcpyDeviceToHost));
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): run the channel alone and return the received samples [B][L][2] and the
// fraction of log / cos values that went to the host's libm.
extern "C" nbl_status nbl_debug_channel(nbl_decoder *d, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B,
                                        double *rx_out, double *flag_frac)
{
	if (!d || !tx_index || !lane_state || !rx_out || B <= 0) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = run_channel(d, tx_index, lane_state, sigma, B, d->stream, &d->d_rx, &d->d_rx_cap, &d->d_gain, &d->d_gain_cap, &d->rx_gain, d->err);
	if (s) return s;
	HIP_TRY(d, hipMemcpyAsync(rx_out, d->d_rx, (size_t)B * d->dm_L * 16, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	if (flag_frac) *flag_frac = d->last_flag_frac;
	return NBL_OK;
}

// Diagnostic only: channel LLRs of codeword b as the decoder holds them, [N][q-1]
extern "C" nbl_status nbl_debug_read_lch(nbl_decoder *d, int32_t b, double *out)
{
	if (!d || !out || b < 0 || b >= d->last_B) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const int q = d->g.q, N = d->g.N;
	double *tmp = nullptr;
	HIP_TRY(d, hipMalloc((void **)&tmp, (size_t)N * (q - 1) * 8));
	HIP_TRY(d, nbl_launch_unpad(d->w.Lch + (size_t)b * N * q, tmp, nullptr, N, q, d->stream));
	HIP_TRY(d, hipMemcpyAsync(out, tmp, (size_t)N * (q - 1) * 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	(void)hipFree(tmp);
	return NBL_OK;
}

extern "C" nbl_status nbl_read_state(nbl_decoder *d, int32_t b, double *post, double *v2c, double *c2v)
{
	if (!d) return NBL_ERR_ARG;
	if (d->idd_sub) { d->err = std::string("nbl_read_state") + IDD_SUB_TEXT; return NBL_ERR_ARG; }
	if (b < 0 || b >= d->last_B) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const int q = d->g.q, N = d->g.N, E = d->g.E;
	double *tmp = nullptr;
	HIP_TRY(d, hipMalloc((void **)&tmp, (size_t)E * (q - 1) * 8));
	nbl_status rc = NBL_OK;
	auto grab = [&](const double *src, const int *map, int rows, double *dst) -> nbl_status {
		HIP_TRY(d, nbl_launch_unpad(src, tmp, map, rows, q, d->stream));
		HIP_TRY(d, hipMemcpyAsync(dst, tmp, (size_t)rows * (q - 1) * 8, hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		return NBL_OK;
	};
	if (post) {
		if (!d->w.post) { d->err = "state recording was off during the last decode (nbl_set_record_state)"; rc = NBL_ERR_ARG; }
		else rc = grab(d->w.post + (size_t)b * N * q, nullptr, N, post);
	}
	if (!rc && v2c) {
		if (d->layered && d->prm.method == NBL_METHOD_EMS) { d->err = "the layered schedule never materialises v2c (a check forms its inputs from L_ch and c2v)"; rc = NBL_ERR_UNSUPPORTED; }
		else if (!d->w.v2c) { d->err = "v2c is not kept in HBM on the fused path unless state recording is on (nbl_set_record_state)"; rc = NBL_ERR_ARG; }
		else rc = grab(d->w.v2c + (size_t)b * E * q, nullptr, E, v2c);
	}
	if (!rc && c2v) {
		const double *src = d->last_c2v ? d->last_c2v : d->w.c2v;
		if (d->last_fused && d->c2v_alt && !d->prm.fixed_iters) {
			// fused iterations: a codeword that converged at iteration k has c2v(k) in one buffer (computed before its syndrome was
			// known) and c2v(k-1), what the reference returns with, intact in the other; iteration i writes bufB when i is odd
			int it = 0;
			uint8_t done = 0;
			HIP_TRY(d, hipMemcpy(&it, d->w.iters + b, sizeof it, hipMemcpyDeviceToHost));
			HIP_TRY(d, hipMemcpy(&done, d->w.done + b, 1, hipMemcpyDeviceToHost));
			if (done) src = (it == 1 && d->c2v_zero) ? d->c2v_zero : ((it - 1) & 1) ? d->c2v_alt : d->w.c2v; // buffer written by iteration it-1 (it = 1: the zeros)
		}
		rc = grab(src == d->c2v_zero ? src : src + (size_t)b * E * q, d->d_e2c_map, E, c2v); // (the zeros are one shared block)
	}
	(void)hipFree(tmp);
	return rc;
}

// Diagnostic only (not part of include/nbldpc.h): the flag-0 OSD posterior sums S of codeword b after the last decode, [N][p]
extern "C" nbl_status nbl_debug_osd_sums(nbl_decoder *d, int32_t b, double *out)
{
	if (!d || !out || b < 0 || b >= d->last_B) return NBL_ERR_ARG;
	if (!d->osd_S) { d->err = "no OSD sums: OSD post-processing with flag 0 is off"; return NBL_ERR_ARG; }
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const size_t n = (size_t)d->g.N * d->g.p;
	HIP_TRY(d, hipMemcpyAsync(out, d->osd_S + (size_t)b * n, n * 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

// ---- transmit side and error count on the device (nbl_tx.hip) ----------------------------------------------------------------

static void free_transmitter(nbl_decoder *d)
{
	nbl_decoder::Tx &t = d->tx;
	if (t.G && t.G != t.T) (void)hipFree(t.G);
	for (void *p : {(void *)t.T, (void *)t.keep, (void *)t.crc_col, (void *)t.phase_of, (void *)t.seq, (void *)t.pn, (void *)t.u, (void *)t.bits,
	                (void *)t.code[0], (void *)t.code[1], (void *)t.txi[0], (void *)t.txi[1], (void *)t.dec[0], (void *)t.dec[1], (void *)t.cnt,
	                (void *)t.e_msg, (void *)t.e_u, (void *)t.e_bits, (void *)t.e_code})
		if (p) (void)hipFree(p);
	t = nbl_decoder::Tx();
}

// one clock of the PN register (Comm.cpp:241-252): shift, then regPN[0] = regPN[10] ^ regPN[3]; the output is regPN[10] after the shift
static inline unsigned pn_step(unsigned s) { return ((s << 1) & 2047u) | (((s >> 9) ^ (s >> 2)) & 1u); }

extern "C" void nbl_pn_advance(uint16_t *state, uint64_t clocks)
{
	if (!state) return;
	// the update is a map of an 11-bit state: square it repeatedly (2048-entry tables) and apply the tables of the set bits
	static const std::vector<std::vector<uint16_t>> pow2 = [] {
		std::vector<std::vector<uint16_t>> t(64, std::vector<uint16_t>(2048));
		for (unsigned s = 0; s < 2048; s++) t[0][s] = (uint16_t)pn_step(s);
		for (int k = 1; k < 64; k++)
			for (unsigned s = 0; s < 2048; s++) t[k][s] = t[k - 1][t[k - 1][s]];
		return t;
	}();
	unsigned s = *state & 2047u;
	for (int k = 0; k < 64; k++)
		if ((clocks >> k) & 1) s = pow2[k][s];
	*state = (uint16_t)s;
}

// tap masks of the CRC registers (Comm.cpp:513-533): bit j set for G[j], j = 0 .. len - 1
static uint32_t crc_tap_mask(int len, int type24)
{
	static const int t8[] = {0, 1, 3, 4, 7}, t16[] = {0, 5, 12}, t24a[] = {0, 1, 3, 4, 5, 6, 7, 10, 11, 14, 17, 18, 23}, t24b[] = {0, 1, 5, 6, 23};
	uint32_t m = 0;
	if (len == 8) for (int x : t8) m |= 1u << x;
	else if (len == 16) for (int x : t16) m |= 1u << x;
	else if (len == 24 && !type24) for (int x : t24a) m |= 1u << x;
	else if (len == 24) for (int x : t24b) m |= 1u << x;
	return m;
}

template <typename T> static nbl_status tx_upload(std::string &err, const std::vector<T> &h, T **dst)
{
	HIP_TRY_E(err, hipMalloc((void **)dst, h.size() * sizeof(T) + 16));
	HIP_TRY_E(err, hipMemcpy(*dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
	return NBL_OK;
}

extern "C" nbl_status nbl_set_transmitter(nbl_decoder *d, const nbl_tx_desc *tx)
{
	if (!d || !tx) return NBL_ERR_ARG;
	d->err.clear();
	const int N = d->g.N, M = d->g.M, q = d->g.q, p = d->g.p, K = N - M;
	if (!d->dm_order) { d->err = "nbl_set_transmitter: nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (d->h_cons.empty() || !d->d_cons) { d->err = "nbl_set_transmitter: the demodulator was set without constellation points (the channel needs them, also for BPSK)"; return NBL_ERR_ARG; }
	if (tx->mod_order != d->dm_order || tx->n_mod_sym != d->dm_L) { d->err = "nbl_set_transmitter: mod_order / n_mod_sym differ from the demodulator's"; return NBL_ERR_ARG; }
	if (tx->mod_order > 256) { d->err = "nbl_set_transmitter: mod_order above 256 is not supported (constellation indices are bytes)"; return NBL_ERR_UNSUPPORTED; }
	if (tx->crc_len != 0 && tx->crc_len != 8 && tx->crc_len != 16 && tx->crc_len != 24) { d->err = "nbl_set_transmitter: crc_len must be 0, 8, 16 or 24"; return NBL_ERR_ARG; }
	if (K <= 0) { d->err = "nbl_set_transmitter: the code has no message symbols"; return NBL_ERR_ARG; }
	if (tx->crc_len > K * p) { d->err = "nbl_set_transmitter: crc_len exceeds the message length K log2(q)"; return NBL_ERR_UNSUPPORTED; }
	if (tx->parallel < 1) { d->err = "nbl_set_transmitter: parallel < 1"; return NBL_ERR_ARG; }
	if (tx->n_punct < 0 || (tx->n_punct > 0 && !tx->punct)) { d->err = "nbl_set_transmitter: bad puncture list"; return NBL_ERR_ARG; }
	for (int i = 0; i < tx->n_punct; i++)
		if (tx->punct[i] < 0 || tx->punct[i] >= N || (i > 0 && tx->punct[i] <= tx->punct[i - 1])) { d->err = "nbl_set_transmitter: punctured positions must be ascending and below N"; return NBL_ERR_ARG; }
	const int mb = ilog2(tx->mod_order);
	// MOD_SYM_LEN = (N - n_punct) p / MOD_BIT_PER_SYM (Comm.cpp:105): the modulator consumes the first L mb kept bits
	if ((long long)tx->n_mod_sym * mb > (long long)(N - tx->n_punct) * p) { d->err = "nbl_set_transmitter: n_mod_sym needs more bits than the unpunctured code word has"; return NBL_ERR_ARG; }
	if (tx->random_msg && !tx->gen) { d->err = "nbl_set_transmitter: gen is NULL with random_msg != 0"; return NBL_ERR_ARG; }
	const int rows = N * p, nb = K * p - tx->crc_len, nw = (nb + 63) / 64, nwg = (K * p + 63) / 64;
	if (rows > 65536 || (size_t)rows * nwg * 8 > ((size_t)64 << 20)) { d->err = "nbl_set_transmitter: code too large for the transmit kernel (N log2(q) above 65536 bits or a matrix above 64 MiB)"; return NBL_ERR_UNSUPPORTED; }
	// H gen = 0 with the decoder's own graph and tables
	if (tx->gen) {
		for (size_t i = 0; i < (size_t)N * K; i++)
			if (tx->gen[i] >= q) { d->err = "nbl_set_transmitter: gen holds a value >= q"; return NBL_ERR_ARG; }
		for (int m = 0; m < M; m++)
			for (int k = 0; k < K; k++) {
				int acc = 0;
				for (int ce = d->h_coff[m]; ce < d->h_coff[m + 1]; ce++) acc ^= d->h_mul[(size_t)d->h_ch[ce] * q + tx->gen[(size_t)d->h_cvar[ce] * K + k]];
				if (acc) { d->err = "nbl_set_transmitter: H * gen != 0 (check " + std::to_string(m) + ", message symbol " + std::to_string(k) + ")"; return NBL_ERR_ARG; }
			}
	}
	HIP_TRY(d, hipSetDevice(d->device));
	if (d->stream2) HIP_TRY(d, hipStreamSynchronize(d->stream2));
	free_transmitter(d);
	nbl_decoder::Tx &t = d->tx;
	t.crc_len = tx->crc_len; t.random_msg = tx->random_msg; t.K = K; t.nb = nb; t.nw = nw; t.nwg = nwg; t.mb = mb;
	nbl_status st;
	if (tx->gen) {
		// G: code bit n p + j as a function of message bit k p + i = bit j of gen[n][k] * x^i, taken from gf_mul itself
		std::vector<unsigned long long> G((size_t)nwg * rows, 0ull);
		for (int n = 0; n < N; n++)
			for (int k = 0; k < K; k++) {
				const int h = tx->gen[(size_t)n * K + k];
				if (!h) continue;
				for (int i = 0; i < p; i++) {
					const int v = d->h_mul[(size_t)h * q + (1 << i)], c = k * p + i;
					for (int j = 0; j < p; j++)
						if ((v >> j) & 1) G[(size_t)(c >> 6) * rows + n * p + j] |= 1ull << (c & 63);
				}
			}
		if ((st = tx_upload(d->err, G, &t.G))) { free_transmitter(d); return st; }
		if (tx->crc_len == 0) t.T = t.G;
		else if (nb > 0) {
			// message bits = [u ; C u]: CRCEncode (type 0) of the unit vector e_i leaves, after the remaining nb - 1 - i zero inputs,
			// the register r_i; r_(nb-1) = taps, r_i = one zero-input clock of r_(i+1).  Parity bit c = register bit len - 1 - c.
			const int len = tx->crc_len;
			const uint32_t taps = crc_tap_mask(len, 0), keepm = (1u << len) - 1u;
			std::vector<uint32_t> r(nb);
			uint32_t reg = taps;
			for (int i = nb - 1; i >= 0; i--) {
				r[i] = reg;
				const uint32_t fb = (reg >> (len - 1)) & 1u;
				reg = ((reg << 1) & keepm) ^ (fb ? taps : 0u);
			}
			std::vector<unsigned long long> T((size_t)nw * rows, 0ull);
			auto gbit = [&](int row, int c) { return (G[(size_t)(c >> 6) * rows + row] >> (c & 63)) & 1ull; };
			for (int row = 0; row < rows; row++) {
				// columns of G at the parity positions, as a register-shaped mask: parity bit c <-> register bit len - 1 - c
				uint32_t pm = 0;
				for (int c = 0; c < len; c++)
					if (gbit(row, nb + c)) pm |= 1u << (len - 1 - c);
				for (int i = 0; i < nb; i++) {
					const unsigned long long b = gbit(row, i) ^ (unsigned long long)(__builtin_popcount(r[i] & pm) & 1);
					if (b) T[(size_t)(i >> 6) * rows + row] |= 1ull << (i & 63);
				}
			}
			if ((st = tx_upload(d->err, T, &t.T))) { free_transmitter(d); return st; }
		}
	}
	{ // kept code bits in modulator order (Puncture, Comm.cpp:290-308)
		std::vector<int> keep;
		int pi = 0;
		for (int n = 0; n < N; n++) {
			if (pi < tx->n_punct && tx->punct[pi] == n) { pi++; continue; }
			for (int j = 0; j < p; j++) keep.push_back(n * p + j);
		}
		keep.resize((size_t)tx->n_mod_sym * mb);
		if ((st = tx_upload(d->err, keep, &t.keep))) { free_transmitter(d); return st; }
	}
	{ // CrcCheck (type 1 for CRC-24) of the K p decoded message bits: remainder of bit i; the last bit enters register bit 0
		std::vector<uint32_t> col((size_t)K * p, 0u);
		if (tx->crc_len) {
			const int len = tx->crc_len;
			const uint32_t taps = crc_tap_mask(len, 1), keepm = (1u << len) - 1u;
			uint32_t reg = 1u;
			for (int i = K * p - 1; i >= 0; i--) {
				col[i] = reg;
				const uint32_t fb = (reg >> (len - 1)) & 1u;
				reg = ((reg << 1) & keepm) ^ (fb ? taps : 0u);
			}
		}
		if ((st = tx_upload(d->err, col, &t.crc_col))) { free_transmitter(d); return st; }
	}
	{ // the register's cycle from the reference's initial contents (Comm.cpp:58-74); a state off the cycle differs from one on it
	  // in regPN[10] only, which no output and no later state depends on
		std::vector<int16_t> phase(2048, -1);
		std::vector<uint8_t> seq;
		unsigned s0 = 0;
		static const int init[11] = {1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1};
		for (int i = 0; i < 11; i++) s0 |= (unsigned)init[i] << i;
		for (unsigned s = s0; phase[s] < 0; s = pn_step(s)) { phase[s] = (int16_t)seq.size(); seq.push_back((uint8_t)((s >> 9) & 1u)); }
		for (unsigned s = 0; s < 2048; s++)
			if (phase[s] < 0 && (s & 1023u)) {
				const unsigned tw = s ^ 1024u;
				if (phase[tw] >= 0) phase[s] = phase[tw];
				else { d->err = "nbl_set_transmitter: internal error, PN register state off its cycle"; free_transmitter(d); return NBL_ERR_ARG; }
			}
		t.period = (int)seq.size();
		t.par_mod = tx->parallel % t.period;
		if ((st = tx_upload(d->err, phase, &t.phase_of)) || (st = tx_upload(d->err, seq, &t.seq))) { free_transmitter(d); return st; }
	}
	t.on = true;
	return NBL_OK;
}

// per-call scratch and the slot's buffers of the channel thread
static nbl_status ensure_tx(nbl_decoder *d, int slot, int B, std::string &err)
{
	nbl_decoder::Tx &t = d->tx;
	const size_t rows = (size_t)d->g.N * d->g.p;
	if ((size_t)B > t.cap) {
		for (void *p : {(void *)t.pn, (void *)t.u, (void *)t.bits})
			if (p) (void)hipFree(p);
		t.pn = nullptr; t.u = nullptr; t.bits = nullptr; t.cap = 0;
		HIP_TRY_E(err, hipMalloc((void **)&t.pn, (size_t)B * 2 + 16));
		HIP_TRY_E(err, hipMalloc((void **)&t.u, (size_t)B * (t.nw > 0 ? t.nw : 1) * 8));
		HIP_TRY_E(err, hipMalloc((void **)&t.bits, (size_t)B * rows));
		t.cap = B;
	}
	if ((size_t)B > t.slot_cap[slot]) {
		for (void *p : {(void *)t.code[slot], (void *)t.txi[slot]})
			if (p) (void)hipFree(p);
		t.code[slot] = nullptr; t.txi[slot] = nullptr; t.slot_cap[slot] = 0;
		HIP_TRY_E(err, hipMalloc((void **)&t.code[slot], (size_t)B * d->g.N));
		HIP_TRY_E(err, hipMalloc((void **)&t.txi[slot], (size_t)B * d->dm_L));
		t.slot_cap[slot] = B;
	}
	return NBL_OK;
}

extern "C" nbl_status nbl_transmit_batch(nbl_decoder *d, int32_t slot, const uint16_t *pn_state, const uint32_t *lane_state, double sigma, int32_t B)
{
	if (!d || !pn_state || !lane_state || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	d->err2.clear();
	if (!d->tx.on) { d->err2 = "nbl_transmit_batch: nbl_set_transmitter has not been called"; return NBL_ERR_ARG; }
	HIP_TRY_E(d->err2, hipSetDevice(d->device));
	if (!d->stream2) HIP_TRY_E(d->err2, hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking));
	nbl_decoder::Tx &t = d->tx;
	d->rxs_B[slot] = 0;
	t.tx_B[slot] = 0;
	nbl_status s = ensure_tx(d, slot, B, d->err2);
	if (s) return s;
	hipStream_t st = d->stream2;
	const int N = d->g.N, p = d->g.p, rows = N * p;
	if (t.random_msg && t.nb > 0) {
		HIP_TRY_E(d->err2, hipMemcpyAsync(t.pn, pn_state, (size_t)B * 2, hipMemcpyHostToDevice, st));
		HIP_TRY_E(d->err2, nbl_launch_tx_pn(t.pn, t.phase_of, t.seq, t.period, t.par_mod, t.nb, t.nw, B, t.u, st));
		HIP_TRY_E(d->err2, nbl_launch_tx_encode(t.T, t.u, rows, t.nw, B, t.bits, st));
	} else {
		HIP_TRY_E(d->err2, hipMemsetAsync(t.bits, 0, (size_t)B * rows, st)); // all-zero message and code word, encoder skipped (Comm.cpp:258-268)
	}
	HIP_TRY_E(d->err2, nbl_launch_tx_pack(t.bits, t.keep, N, p, d->dm_L, t.mb, B, t.code[slot], t.txi[slot], st));
	s = run_channel(d, nullptr, lane_state, sigma, B, st, &d->d_rxs[slot], &d->d_rxs_cap[slot], &d->d_gains[slot], &d->d_gains_cap[slot],
	                &d->slot_gain[slot], d->err2, t.txi[slot]);
	if (s == NBL_OK) { d->rxs_B[slot] = B; t.tx_B[slot] = B; }
	return s;
}

extern "C" nbl_status nbl_count_errors(nbl_decoder *d, int32_t slot, int32_t B, int32_t *err_sym, int32_t *err_bit, uint8_t *crc_ok)
{
	if (!d || B <= 0 || slot < 0 || slot > 1 || !err_sym || !err_bit || !crc_ok) return NBL_ERR_ARG;
	d->err.clear();
	nbl_decoder::Tx &t = d->tx;
	if (!t.on) { d->err = "nbl_count_errors: nbl_set_transmitter has not been called"; return NBL_ERR_ARG; }
	if (t.tx_B[slot] != B) { d->err = "nbl_count_errors: slot does not hold a transmitted batch of this size (nbl_transmit_batch first)"; return NBL_ERR_ARG; }
	if (t.dec_B[slot] != B) { d->err = "nbl_count_errors: slot does not hold the outputs of a decode of this size (nbl_decode_batch_resident first)"; return NBL_ERR_ARG; }
	HIP_TRY(d, hipSetDevice(d->device));
	if ((size_t)B > t.cnt_cap) {
		if (t.cnt) (void)hipFree(t.cnt);
		t.cnt = nullptr; t.cnt_cap = 0;
		HIP_TRY(d, hipMalloc((void **)&t.cnt, (size_t)B * 9 + 16));
		t.cnt_cap = B;
	}
	int *es = t.cnt, *eb = t.cnt + t.cnt_cap;
	uint8_t *ok = (uint8_t *)(t.cnt + 2 * t.cnt_cap);
	HIP_TRY(d, nbl_launch_tx_errcount(t.dec[slot], t.code[slot], t.crc_col, d->g.N, t.K, d->g.p, t.crc_len, B, es, eb, ok, d->stream));
	HIP_TRY(d, hipMemcpyAsync(err_sym, es, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipMemcpyAsync(err_bit, eb, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipMemcpyAsync(crc_ok, ok, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_encode_batch(nbl_decoder *d, const int32_t *msg, int32_t B, int32_t *code, int32_t *msg_out)
{
	if (!d || !msg || !code || B < 0) return NBL_ERR_ARG;
	d->err.clear();
	nbl_decoder::Tx &t = d->tx;
	if (!t.on || !t.G) { d->err = "nbl_encode_batch: nbl_set_transmitter has not been called with a generator"; return NBL_ERR_ARG; }
	if (B == 0) return NBL_OK;
	const int N = d->g.N, p = d->g.p, K = t.K, rows = N * p, q = d->g.q;
	for (size_t i = 0; i < (size_t)B * K; i++)
		if (msg[i] < 0 || msg[i] >= q) { d->err = "nbl_encode_batch: message symbol outside 0 .. q - 1"; return NBL_ERR_ARG; }
	HIP_TRY(d, hipSetDevice(d->device));
	const int chunk = B < 4096 ? B : 4096;
	if ((size_t)chunk > t.e_cap) {
		for (void *x : {(void *)t.e_msg, (void *)t.e_u, (void *)t.e_bits, (void *)t.e_code})
			if (x) (void)hipFree(x);
		t.e_msg = nullptr; t.e_u = nullptr; t.e_bits = nullptr; t.e_code = nullptr; t.e_cap = 0;
		HIP_TRY(d, hipMalloc((void **)&t.e_msg, (size_t)chunk * K * 4));
		HIP_TRY(d, hipMalloc((void **)&t.e_u, (size_t)chunk * t.nwg * 8));
		HIP_TRY(d, hipMalloc((void **)&t.e_bits, (size_t)chunk * rows));
		HIP_TRY(d, hipMalloc((void **)&t.e_code, (size_t)chunk * N));
		t.e_cap = chunk;
	}
	std::vector<uint8_t> h((size_t)chunk * N);
	for (int b0 = 0; b0 < B; b0 += chunk) {
		const int n = B - b0 < chunk ? B - b0 : chunk;
		HIP_TRY(d, hipMemcpyAsync(t.e_msg, msg + (size_t)b0 * K, (size_t)n * K * 4, hipMemcpyHostToDevice, d->stream));
		HIP_TRY(d, nbl_launch_tx_msgbits(t.e_msg, K, p, t.nwg, n, t.e_u, d->stream));
		HIP_TRY(d, nbl_launch_tx_encode(t.G, t.e_u, rows, t.nwg, n, t.e_bits, d->stream));
		// (symbols only: the index output goes to the same buffer's tail-less twin with L = 0)
		HIP_TRY(d, nbl_launch_tx_pack(t.e_bits, t.keep, N, p, 0, t.mb, n, t.e_code, nullptr, d->stream));
		HIP_TRY(d, hipMemcpyAsync(h.data(), t.e_code, (size_t)n * N, hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		for (int b = 0; b < n; b++) {
			for (int i = 0; i < N; i++) code[(size_t)(b0 + b) * N + i] = h[(size_t)b * N + i];
			if (msg_out) for (int i = 0; i < K; i++) msg_out[(size_t)(b0 + b) * K + i] = h[(size_t)b * N + i];
		}
	}
	return NBL_OK;
}

extern "C" nbl_status nbl_read_transmitted(nbl_decoder *d, int32_t slot, int32_t b0, int32_t n, int32_t *tx_msg, int32_t *tx_code, uint8_t *tx_index)
{
	if (!d || slot < 0 || slot > 1 || b0 < 0 || n < 0) return NBL_ERR_ARG;
	d->err.clear();
	nbl_decoder::Tx &t = d->tx;
	if (!t.on || t.tx_B[slot] <= 0 || (long long)b0 + n > t.tx_B[slot]) { d->err = "nbl_read_transmitted: the slot does not hold these lanes (nbl_transmit_batch first)"; return NBL_ERR_ARG; }
	if (n == 0) return NBL_OK;
	HIP_TRY(d, hipSetDevice(d->device));
	const int N = d->g.N, K = t.K, L = d->dm_L;
	if (tx_msg || tx_code) {
		std::vector<uint8_t> h((size_t)n * N);
		HIP_TRY(d, hipMemcpy(h.data(), t.code[slot] + (size_t)b0 * N, h.size(), hipMemcpyDeviceToHost));
		for (int b = 0; b < n; b++) {
			if (tx_code) for (int i = 0; i < N; i++) tx_code[(size_t)b * N + i] = h[(size_t)b * N + i];
			if (tx_msg) for (int i = 0; i < K; i++) tx_msg[(size_t)b * K + i] = h[(size_t)b * N + i];
		}
	}
	if (tx_index) HIP_TRY(d, hipMemcpy(tx_index, t.txi[slot] + (size_t)b0 * L, (size_t)n * L, hipMemcpyDeviceToHost));
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): the received samples [n][L][2] a slot holds
extern "C" nbl_status nbl_debug_read_slot_rx(nbl_decoder *d, int32_t slot, int32_t b0, int32_t n, double *rx)
{
	if (!d || slot < 0 || slot > 1 || b0 < 0 || n <= 0 || !rx || b0 + n > d->rxs_B[slot]) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	HIP_TRY(d, hipMemcpy(rx, d->d_rxs[slot] + (size_t)b0 * d->dm_L * 2, (size_t)n * d->dm_L * 16, hipMemcpyDeviceToHost));
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): put decoded words [B][N] where nbl_decode_batch_resident leaves a slot's outputs
extern "C" nbl_status nbl_debug_set_decoded(nbl_decoder *d, int32_t slot, const int32_t *sym, int32_t B)
{
	if (!d || slot < 0 || slot > 1 || !sym || B <= 0) return NBL_ERR_ARG;
	d->err.clear();
	if (!d->tx.on) { d->err = "nbl_debug_set_decoded: nbl_set_transmitter has not been called"; return NBL_ERR_ARG; }
	HIP_TRY(d, hipSetDevice(d->device));
	d->tx.dec_B[slot] = 0;
	nbl_status s = ensure_slot_dec(d, slot, B);
	if (s) return s;
	HIP_TRY(d, hipMemcpy(d->tx.dec[slot], sym, (size_t)B * d->g.N * 4, hipMemcpyHostToDevice));
	d->tx.dec_B[slot] = B;
	return NBL_OK;
}
